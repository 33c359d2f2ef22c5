"""Tube-light attack on the object patch: the black-box random search of the reference's ``evaluate_attacks``
(``MD2/evaluate_depth.py:150-151,178-182``, ``norm_type == "light"``).

Same class name, constructor, call signature and return tuple as the reference's ``torchattacks/attacks/phy_obj_atk_light.py``
(forward :64-188); the literals 200 and 20 of :113 and :88 are the keywords ``n_init`` and ``n_search``.  The search casts
n_init x n_search x 2 coloured light beams on the object, pastes each lit object at fresh random poses, and keeps the one the
model answers with the smallest masked disparity.  Nothing in it depends on the model's answers -- ``init_v`` is never updated
(:117-128), the only feedback is the running minimum (:165-167) -- so every parameter set (numpy's generator) and every pose
(Python's) is drawn on the host before the first launch, in the reference's order, and the loop reads nothing back:

    per query   K24 tube_light_compose (the lit patch, from the record the device cursor points at)
                -> K3 eot_paste -> model / K19 windowed cost -> K24 tube_light_commit (cost array, best cost, best query, cursor)

where the reference fills a 260 x 300 x 3 array in a Python double loop, adds it with OpenCV, rounds through a PIL uint8 image,
uploads it and compares the cost with the best so far on the host, 8000 times.  After the loop the best patch is regenerated
from the best query's record by the same kernel (deterministic: the very bits that won).
"""
import numpy as np
import torch

from ... import ops
from ...my_utils import to_device_async
from .object_search import _ObjectSearch

Q = np.asarray([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1, 1, 0, 0], [1, 0, 1, 0], [1, 0, 0, 1], [0, 1, 1, 0],
                [0, 1, 0, 1], [0, 0, 1, 1]])        # the search directions of :90-100: wavelength, angle, b, beta
LO, HI = [380, 0, 0, 10], [750, 180, 400, 1600]     # :128


class Phy_obj_atk_light(_ObjectSearch):
    r"""
    Arguments:
        model (nn.Module): model to attack.
        obj_img (1x3xHxW), obj_mask (1x1xHxW): object patch and its paint mask.
        eps, alpha, steps, random_start: accepted as the reference accepts them; the search does not use them.
        n_init (int): start points of the search. (Default: 200)
        n_search (int): random directions per start point, each tried both ways. (Default: 20)
        host_chain (bool): run the reference's shape instead -- the pattern in numpy on the host, an upload and a host
            comparison per query -- on the same paste / cost kernels (the benchmark's baseline and the tests' eager twin).
    """

    def __init__(self, model, obj_img, obj_mask, eps=1, alpha=0.2, steps=40, random_start=True,
                 dist_range=list(range(5, 31, 2)), n_init=200, n_search=20, host_chain=False):
        super().__init__(model, obj_img, obj_mask, host_chain=host_chain, eps=eps, alpha=alpha, steps=steps,
                         random_start=random_start, dist_range=dist_range)
        if int(n_init) < 1 or int(n_search) < 1:
            raise ValueError("Phy_obj_atk_light: n_init and n_search must be positive")
        self.n_init, self.n_search = int(n_init), int(n_search)
        # trace (see _ObjectSearch): params = (wavelength, angle, b, beta)

    def draw_params(self):
        """int64 [n_init * n_search * 2, 4]: every parameter set of the search from numpy's global generator in the order of
        :113-128 (all start points first; per direction one ``randint(len(Q))`` and one ``randint(1, 20)``, used for a = -1, +1)."""
        inits = [[np.random.randint(380, 750), np.random.randint(0, 180), np.random.randint(0, 400), np.random.randint(10, 1600)]
                 for _ in range(self.n_init)]
        out = np.zeros((self.n_init, self.n_search, 2, 4), dtype=np.int64)
        for i, init_v in enumerate(inits):
            for s in range(self.n_search):
                q = Q[np.random.randint(len(Q))] * np.random.randint(1, 20)
                for j, a in enumerate((-1, 1)):
                    out[i, s, j] = np.clip(np.asarray(init_v) + a * q, LO, HI)
        return out.reshape(-1, 4)

    def _prepare(self, obj):
        """numpy's stream first (:113-128), as the reference draws it; ``base``: ToPILImage (:111), truncation."""
        params = self.draw_params()
        return len(params), (params, ops.tube_light_table(params), obj.mul(255).to(torch.uint8).contiguous())

    def _device_search(self, obj, n, ctx):
        _, table_host, base = ctx
        table = to_device_async(table_host, self.device)
        return ops.tube_light_state(n, self.device), lambda cursor, out: ops.tube_light_compose(table, cursor, base, out=out)

    def _host_patches(self, obj, ctx):
        """The pattern on the host (numpy, where the reference loops in Python), then ToTensor and the upload."""
        _, table_host, base = ctx
        base_hwc = base[0].permute(1, 2, 0).contiguous().cpu().numpy()

        def make(q):
            u8 = ops.tube_light_host(base_hwc, table_host[q])
            return torch.from_numpy(u8).permute(2, 0, 1).float().div(255).unsqueeze(0).to(self.device).contiguous()
        return make

    def _trace_fields(self, ctx, q):
        return dict(params=tuple(int(v) for v in ctx[0][q]))
