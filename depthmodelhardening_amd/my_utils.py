"""Globals of the reference's root ``my_utils.py`` that are part of the hot-path boundary.

Reference: my_utils.py:10-14 (device0, object_dataset_root, ori_H, ori_W, train_dist_range),
:19-41 (disp_to_depth, get_mean_depth_diff), :43-105,128-137 (eval_depth_diff, eval_depth_diff_jcl, save_pic: the figures,
composed on the device through K37, ops.disp_colorize).
"""
import os

import numpy as np
import torch

# my_utils.py:11 hard-codes the authors' machine; here it is overridable and may not exist at all
object_dataset_root = os.environ.get("DMH_KITTI_OBJECT_ROOT", "/data3/share/kitti/object/")
ori_H = 375
ori_W = 1242
train_dist_range = list(np.arange(5, 10, 0.2))

# P2 of KITTI-object calib 003086 (first two rows are quoted in physicalTrans.py:208-213): used when
# ``{object_dataset_root}/training/calib/003086.txt`` is not on disk (synthetic-data runs).
KITTI_003086_P2 = np.array([[7.215377e+02, 0.0, 6.095593e+02, 4.485728e+01],
                            [0.0, 7.215377e+02, 1.728540e+02, 2.163791e-01],
                            [0.0, 0.0, 1.0, 2.745884e-03]], dtype=np.float64)


def disp_to_depth(disp, min_depth, max_depth):
    """my_utils.py:19-29 (same as MD2/layers.py:16-25)."""
    min_disp = 1 / max_depth
    max_disp = 1 / min_depth
    scaled_disp = min_disp + (max_disp - min_disp) * disp
    depth = 1 / scaled_disp
    return scaled_disp, depth


def get_mean_depth_diff(adv_disp1, ben_disp2, scene_car_mask=None, use_abs=False):
    """my_utils.py:31-41."""
    scaler = 5.4
    if scene_car_mask is None:
        scene_car_mask = torch.ones_like(adv_disp1)
    dep1_adv = torch.clamp(disp_to_depth(torch.abs(adv_disp1), 0.1, 100)[1] * scene_car_mask * scaler, max=100)
    dep2_ben = torch.clamp(disp_to_depth(torch.abs(ben_disp2), 0.1, 100)[1] * scene_car_mask * scaler, max=100)
    if use_abs:
        return torch.sum(torch.abs(dep1_adv - dep2_ben)) / torch.sum(scene_car_mask)
    return torch.sum(dep1_adv - dep2_ben) / torch.sum(scene_car_mask)


def to_device_async(data, device, dtype=None):
    """Small host array / list -> device tensor WITHOUT a host synchronisation: staged through pinned memory and
    copied asynchronously on the current stream.  A pageable `tensor.to(device)` makes the host wait until the GPU has
    drained its queue; the GPU then idles while the host prepares the next launches (measured: five such stalls of
    ~1.8 ms per training step)."""
    import numpy as np
    import torch
    t = torch.from_numpy(np.ascontiguousarray(data)) if isinstance(data, np.ndarray) else torch.as_tensor(data)
    if dtype is not None:
        t = t.to(dtype)
    device = torch.device(device)
    if device.type == "cuda":
        return t.pin_memory().to(device, non_blocking=True)
    return t.to(device)


# ------------------------------------------------------------------------------------------ figures (my_utils.py:43-105,128-137)
FIGURE_GAP = 8          # pixels between the panels of a figure and around them
FIGURE_FILL = 255       # the background byte (matplotlib's white figure)


def _to_pil_bytes(img):
    """transforms.ToPILImage()(img.squeeze()) of a float image [.., 3, H, W] in [0, 1] as uint8 [H, W, 3]: mul(255), then the
    truncating cast.  Values outside [0, 1], which ``.byte()`` would wrap, are clamped first."""
    img = img.detach()
    while img.dim() > 3:
        if img.shape[0] != 1:
            raise RuntimeError("figure: one image per panel; got a batch of shape %s" % (tuple(img.shape),))
        img = img[0]
    if img.dim() != 3 or img.shape[0] != 3:
        raise RuntimeError("figure: an image panel is [3, H, W]; got %s" % (tuple(img.shape),))
    return img.clamp(0, 1).mul(255).to(torch.uint8).permute(1, 2, 0)


def _disp_map(disp, img, depth_model):
    """The panel's disparity [h, w] float32: ``disp`` squeezed, or depth_model(img) (my_utils.py:44-51)."""
    if disp is None:
        with torch.no_grad():
            disp = depth_model(img if img.dim() == 4 else img[None])
    disp = disp.detach().float()
    while disp.dim() > 2:
        if disp.shape[0] != 1:
            raise RuntimeError("figure: one disparity map per panel; got shape %s" % (tuple(disp.shape),))
        disp = disp[0]
    return disp


def figure_layout(img_hw, disp_hw, jcl=False):
    """The mosaic's geometry: (height, width, image origins, colour-panel origins), (y, x) each.  Rows of an image panel (both
    images side by side; the first only with ``jcl``) and of the colour panels -- 3 x 2 as my_utils.py:58-67, 3 x 1 as :90-97 --
    at native resolution, ``FIGURE_GAP`` pixels apart."""
    (ih, iw), (dh, dw), gp = img_hw, disp_hw, FIGURE_GAP
    cols = 1 if jcl else 2
    cw = max(iw, dw)
    width = gp + cols * (cw + gp)
    xs = [gp + c * (cw + gp) for c in range(cols)]
    y1 = gp + ih + gp
    if jcl:
        colour = [(y1, xs[0]), (y1 + dh + gp, xs[0])]
    else:
        colour = [(y1, xs[0]), (y1, xs[1]), (y1 + dh + gp, xs[0]), (y1 + dh + gp, xs[1])]
    return y1 + 2 * (dh + gp), width, [(gp, x) for x in xs], colour


def _figure(img1, img2, depth_model, disp1, disp2, jcl):
    from . import ops
    disp1, disp2 = _disp_map(disp1, img1, depth_model), _disp_map(disp2, img2, depth_model)
    if disp1.shape != disp2.shape or disp1.device != disp2.device:
        raise RuntimeError("figure: the two disparity maps must share a shape and a device; got %s and %s"
                           % (tuple(disp1.shape), tuple(disp2.shape)))
    images = [_to_pil_bytes(img1)] + ([] if jcl else [_to_pil_bytes(img2)])
    height, width, img_at, colour_at = figure_layout(tuple(images[0].shape[:2]), tuple(disp1.shape), jcl)
    dev = disp1.device
    mosaic = torch.full((height, width, 3), FIGURE_FILL, dtype=torch.uint8, device=dev)
    for im, (y, x) in zip(images, img_at):
        mosaic[y:y + im.shape[0], x:x + im.shape[1]] = im.to(dev)
    # my_utils.py:55,61-67: vmax = the 95th percentile of disparity 1 for panels 3-5, imshow's autoscale for panel 6
    panels = [(0, -1, "zero_ref", 0)] + (
        [(0, 1, "zero_ref", 0)] if jcl else [(1, -1, "zero_ref", 0), (0, 1, "zero_ref", 0), (0, 1, "min_max", 3)])
    ops.disp_colorize(torch.stack([disp1, disp2]), panels, out=mosaic, origins=colour_at)
    return mosaic, disp1, disp2


def _figure_image(mosaic, filename):
    from PIL import Image
    image = Image.fromarray(mosaic.cpu().numpy())        # the one copy to the host
    if filename is not None:
        image.save('temp_' + filename + '.png')
    return image


def eval_depth_diff(img1, img2, depth_model, filename=None, disp1=None, disp2=None):
    """my_utils.py:43-73 as a plain mosaic composed on the device at native resolution: image 1 | image 2, disparity 1 |
    disparity 2 (magma, 0 .. the 95th percentile of disparity 1), |disparity 1 - disparity 2| under the same limits | the same
    difference under its own minimum and maximum.  It is NOT matplotlib's rendered figure: no titles, no axes, no resampling to a
    12 x 7 inch canvas -- every colour byte is the byte ``imshow`` maps that pixel's value to.  One K37 call writes the four colour
    panels into their places, the image panels are copied beside them, and the mosaic is read back once.
    Returns (PIL image, disp1, disp2), the disparities as numpy arrays [h, w] as the reference returns them."""
    mosaic, disp1, disp2 = _figure(img1, img2, depth_model, disp1, disp2, jcl=False)
    return _figure_image(mosaic, filename), disp1.cpu().numpy(), disp2.cpu().numpy()


def eval_depth_diff_jcl(img1, img2, depth_model, filename=None, disp1=None, disp2=None):
    """my_utils.py:75-105: the three-row form -- image 1, disparity 1, the disparity difference (0 .. the 95th percentile of
    disparity 1) -- as the same kind of mosaic as ``eval_depth_diff``.  Returns the PIL image."""
    mosaic, _, _ = _figure(img1, img2, depth_model, disp1, disp2, jcl=True)
    return _figure_image(mosaic, filename)


def save_pic(tensor, i, log_dir=''):
    """my_utils.py:128-137: a [1, 3, H, W] (or [3, H, W]) image in [0, 1] as ``<log_dir>/<i>.png``."""
    from PIL import Image
    image = Image.fromarray(_to_pil_bytes(tensor.cpu().clone()).contiguous().numpy())
    file_path = os.path.join(log_dir, "{}.png".format(i)) if log_dir != '' else "{}.png".format(i)
    image.save(file_path, "PNG")
