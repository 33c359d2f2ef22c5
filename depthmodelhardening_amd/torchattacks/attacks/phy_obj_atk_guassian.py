"""Gaussian-blur attack on the object patch: the gradient-free search over growing sigmas of the reference's
``evaluate_attacks`` (``MD2/evaluate_depth.py:148-149``, ``norm_type == "guassian"``, the reference's spelling).

Same class name, constructor, call signature and return tuple as the reference's ``torchattacks/attacks/phy_obj_atk_guassian.py``
(forward :61-141).  For ``steps`` growing sigmas the reference blurs the whole object with ``scipy.ndimage.gaussian_filter`` on
the host, writes the blurred rectangle [90:170, 100:200] into the object, pastes it at fresh random poses and keeps the step the
model answers with the smallest masked disparity.  Nothing in it depends on the model's answers -- the mask is 0 / 1, so the
accumulated patch is always "this step's blur inside the rectangle, the original outside" -- so every blurred rectangle is made
by K26 before the search (two launches for all steps, bit-equal to scipy), every pose is drawn on the host up front in the
reference's order, and the loop reads nothing back:

    per step    K26 gauss_blur_compose (the window the device cursor points at, into the object)
                -> K3 eot_paste -> model / K19 windowed cost -> K24 tube_light_commit (cost array, best cost, best step, cursor)

After the loop the best patch is recomposed from the best step's window by the same kernel.
"""
import torch

from ... import ops
from ...my_utils import to_device_async
from .object_search import _ObjectSearch


class Phy_obj_atk_guassian(_ObjectSearch):
    r"""
    Arguments:
        model (nn.Module): model to attack.
        obj_img (1x3xHxW), obj_mask (1x1xHxW): object patch and its paint mask.
        steps (int): number of sigmas tried; step i blurs with sigma (i / steps) (max(H, W) // 2). (Default: 40)
        eps, alpha, random_start: accepted as the reference accepts them; the search does not use them.
        region (r0, r1, c0, c1): the rectangle of the object that is repainted, clipped as the slices clip.
            (Default: the reference's (90, 170, 100, 200))
        host_chain (bool): run the reference's shape instead -- the blur in numpy on the host, an upload and a host
            comparison per step -- on the same paste / cost kernels (the benchmark's baseline and the tests' eager twin).
    """

    noun = "step"

    def __init__(self, model, obj_img, obj_mask, eps=1, alpha=0.2, steps=40, random_start=True,
                 dist_range=list(range(5, 31, 2)), region=ops.GAUSS_REGION, host_chain=False):
        super().__init__(model, obj_img, obj_mask, host_chain=host_chain, eps=eps, alpha=alpha, steps=steps,
                         random_start=random_start, dist_range=dist_range)
        if int(steps) < 1:
            raise RuntimeError("Phy_obj_atk_guassian: steps must be positive")
        self.alpha = 2.5 * eps / steps      # :45
        self.region = tuple(int(v) for v in region)
        # trace (see _ObjectSearch): sigma

    def _prepare(self, obj):
        h, w = int(obj.shape[-2]), int(obj.shape[-1])
        sigmas = ops.gauss_sigmas(int(self.steps), h, w)
        rect = ops._gauss_region(self.region, h, w, "Phy_obj_atk_guassian")       # an empty rectangle: refused before any draw
        return len(sigmas), (sigmas, rect)

    def _device_search(self, obj, n, ctx):
        weights_host, radii_host = ops.gauss_blur_table(ctx[0])
        weights, radii = to_device_async(weights_host, self.device), to_device_async(radii_host, self.device)
        search = ops.tube_light_state(n, self.device)
        with torch.no_grad():
            windows = ops.gauss_blur_windows(obj, weights, radii, self.region)     # every step's rectangle: two launches
        return search, lambda cursor, out: ops.gauss_blur_compose(windows, cursor, obj, self.region, out=out)

    def _host_patches(self, obj, ctx):
        """The blur on the host (numpy in scipy's order, the rectangle only), the upload, the rectangle written into the object."""
        sigmas, (r0, r1, c0, c1) = ctx
        x0 = obj.cpu().numpy()      # :81

        def make(q):
            window = torch.from_numpy(ops.gauss_blur_host(x0, sigmas[q], self.region)).to(self.device)
            patch = obj.clone()
            patch[:, :, r0:r1, c0:c1] = window
            return patch
        return make

    def _trace_fields(self, ctx, q):
        return dict(sigma=ctx[0][q])
