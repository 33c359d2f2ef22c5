"""The update kernels of the evaluation attacks (K20-K28): the L_inf and L2 steps, the APGD controller, the tube-light, Gaussian-blur
and Square searches and the L0 nodes.  Stateless; ops.py re-exports every name, and callers reach them as ``ops.<name>``.

The operators launch on the device only.  The ``*_host`` functions are the exception: each is the numpy restatement its kernel
is held to, and runs on host arrays and CPU tensors.
"""
import numpy as np
import torch

from . import _native as N
from ._launch import _c, _need_cuda


def pgd_linf_step(x, x0, grad, alpha, eps, out=None):
    """x <- clamp(x0 + clamp(x + alpha*sign(grad) - x0, -eps, eps), 0, 1) (phy_obj_atk.py:98-101)."""
    x, x0, grad = _c(x.detach()), _c(x0), _c(grad)
    if x.shape != x0.shape or x.shape != grad.shape:
        raise RuntimeError("pgd_linf_step: shape mismatch")
    if out is None:
        out = torch.empty_like(x)
    N.check(N.lib().dmh_pgd_linf_step(N.ptr(x), N.ptr(x0), N.ptr(grad), float(alpha), float(eps), N.ptr(out),
                                      x.numel(), N.stream()))
    return out


def pgd_l2_workspace(n, device):
    """The float64 workspace of pgd_l2_step for tensors of ``n`` elements: K28's per-workgroup partial sums."""
    return torch.empty(int(N.lib().dmh_pgd_l2_workspace_size(int(n))) // 8, device=device, dtype=torch.float64)


def pgd_l2_step(x, x0, grad, alpha, eps, out=None, workspace=None):
    """K28: y = x + alpha grad / (||grad||_2 + 1e-10); out = clamp(x0 + (y - x0) min(eps / ||y - x0||_2, 1), 0, 1), with ONE norm
    over the whole tensor (phy_obj_atk_l2.py:110-120, shared-patch form).  Two launches, no host read.  ``workspace``:
    pgd_l2_workspace(x.numel(), x.device), written by every call (one is allocated when none is given: not inside a graph capture
    that is to be replayed).  ``out`` must be a tensor of its own."""
    x, x0, grad = _c(x.detach()), _c(x0), _c(grad)
    if x.shape != x0.shape or x.shape != grad.shape:
        raise RuntimeError("pgd_l2_step: shape mismatch")
    if not float(eps) >= 0.0:
        raise RuntimeError("pgd_l2_step: eps must not be negative")
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape:
        raise RuntimeError("pgd_l2_step: shape mismatch")
    if workspace is None:
        workspace = pgd_l2_workspace(x.numel(), x.device)
    N.check(N.lib().dmh_pgd_l2_step(N.ptr(x), N.ptr(x0), N.ptr(grad), float(alpha), float(eps), N.ptr(out), x.numel(),
                                    N.ptr_f64(workspace), workspace.numel() * 8, N.stream()))
    return out


APGD_REC = 16       # floats per controller record (DMH_APGD_REC)


def apgd_controller(steps, eps, loss0, rho=0.75):
    """Device state of the Auto-PGD controller (K22) for one attack of ``steps`` iterations: (ctl [steps + 1, 16] with record 0
    filled from phy_obj_atk_apgd.py:137,190-200, hist [steps] zeros, cursor int32 [2] zeros, size_decr, steps_min).  ``loss0``:
    the device scalar holding the loss at the start point (loss_best and loss_best_last_check start there); nothing is read back."""
    steps = int(steps)
    if steps < 1 or steps >= 1 << 24:
        raise RuntimeError("apgd_controller: steps must lie in [1, 2^24)")
    _need_cuda(loss0)
    k0, steps_min, size_decr = max(int(0.22 * steps), 1), max(int(0.06 * steps), 1), max(int(0.03 * steps), 1)
    host = torch.zeros((steps + 1, APGD_REC), dtype=torch.float32)
    host[0, 0], host[0, 1], host[0, 4], host[0, 7] = 2.0 * float(torch.tensor(eps, dtype=torch.float32)), 1.0, k0, 1.0
    ctl = host.to(loss0.device, non_blocking=True)
    ctl[0, 2:4] = loss0.detach().reshape(1).to(torch.float32)
    hist = torch.zeros(steps, device=loss0.device, dtype=torch.float32)
    cursor = torch.zeros(2, device=loss0.device, dtype=torch.int32)
    return ctl, hist, cursor, size_decr, steps_min


def _apgd_check(name, steps, ctl, hist, cursor, tensors):
    n = tensors[0].numel()
    for t in tensors:
        if t.numel() != n or t.dtype != torch.float32:
            raise RuntimeError("%s: the patch-sized tensors must be fp32 and of one size" % name)
    if int(steps) < 1 or ctl.dtype != torch.float32 or ctl.numel() < (int(steps) + 1) * APGD_REC:
        raise RuntimeError("%s: ctl must hold steps + 1 records of %d floats" % (name, APGD_REC))
    if hist is not None and (hist.dtype != torch.float32 or hist.numel() < int(steps)):
        raise RuntimeError("%s: hist must hold steps floats" % name)
    if cursor.dtype != torch.int32 or cursor.numel() < 2:
        raise RuntimeError("%s: cursor must be int32[2]" % name)
    return n


def apgd_step(x_adv, x_old, x0, grad, ctl, cursor, steps, eps):
    """In place: x_old <- x_adv, x_adv <- Auto-PGD's momentum step (phy_obj_atk_apgd.py:207-215) with the step size and the
    momentum weight of the controller record the device cursor points at.  No host value of the iteration enters."""
    n = _apgd_check("apgd_step", steps, ctl, None, cursor, (x_adv, x_old, x0, grad))
    N.check(N.lib().dmh_apgd_step(N.ptr(x_adv), N.ptr(x_old), N.ptr(x0), N.ptr(grad), N.ptr(ctl), N.ptr(cursor), int(steps),
                                  float(eps), n, N.stream()))
    return x_adv


def apgd_commit(x_adv, g_new, grad, x_best, grad_best, x_ret, loss, ctl, hist, cursor, steps, size_decr, steps_min, rho=0.75):
    """In place, decided on the device from ``loss`` (device scalar: the cost at the new x_adv, ``g_new`` its gradient) and the
    controller record: best point, loss history, checkpoint, step halving, restart (phy_obj_atk_apgd.py:255-290); writes the
    next record and advances the cursor."""
    n = _apgd_check("apgd_commit", steps, ctl, hist, cursor, (x_adv, g_new, grad, x_best, grad_best, x_ret))
    if loss.numel() != 1 or loss.dtype != torch.float32:
        raise RuntimeError("apgd_commit: loss must be one fp32 value")
    N.check(N.lib().dmh_apgd_commit(N.ptr(x_adv), N.ptr(g_new), N.ptr(grad), N.ptr(x_best), N.ptr(grad_best), N.ptr(x_ret),
                                    N.ptr(loss), N.ptr(ctl), N.ptr(hist), N.ptr(cursor), int(steps), int(size_decr),
                                    int(steps_min), float(rho), n, N.stream()))
    return x_adv


LIGHT_REC = 10      # doubles per query record (DMH_LIGHT_REC)


def tube_light_table(params, alpha=1.0):
    """Host: the record array [n, 10] float64 of K24 for ``params`` [n, 4] = (wavelength, angle, b, beta) per query.  Every scalar
    is made in float64 the way the reference's Python makes it: k = round(tan(radians(angle)), 2) (phy_obj_atk_light.py:130-131),
    full_end = int(sqrt(beta) + 0.5), light_end = int(sqrt(beta * 20) + 0.5), the divisor sqrt(1 + k k) and the colour of
    wavelength_to_rgb with its ``** 0.8`` times alpha (light_simulation.py:40-84,143-146,150)."""
    import math
    params = np.asarray(params).reshape(-1, 4)
    out = np.zeros((len(params), LIGHT_REC), dtype=np.float64)
    for row, (wl, angle, b, beta) in zip(out, params.tolist()):
        k = round(math.tan(math.radians(angle)), 2)
        w, g = float(wl), 0.8
        if 380 <= w <= 440:         # the first matching band wins at a shared boundary
            att = 0.3 + 0.7 * (w - 380) / (440 - 380)
            c = (((-(w - 440) / (440 - 380)) * att) ** g, 0.0, (1.0 * att) ** g)
        elif 440 <= w <= 490:
            c = (0.0, ((w - 440) / (490 - 440)) ** g, 1.0)
        elif 490 <= w <= 510:
            c = (0.0, 1.0, (-(w - 510) / (510 - 490)) ** g)
        elif 510 <= w <= 580:
            c = (((w - 510) / (580 - 510)) ** g, 1.0, 0.0)
        elif 580 <= w <= 645:
            c = (1.0, (-(w - 645) / (645 - 580)) ** g, 0.0)
        elif 645 <= w <= 750:
            c = ((1.0 * (0.3 + 0.7 * (750 - w) / (750 - 645))) ** g, 0.0, 0.0)
        else:
            c = (0.0, 0.0, 0.0)
        row[:9] = (k, b, beta, int(math.sqrt(beta) + 0.5), int(math.sqrt(beta * 20) + 0.5), math.sqrt(1 + k * k),
                   c[0] * alpha, c[1] * alpha, c[2] * alpha)
    return out


def tube_light_host(base_hwc, rec):
    """Host twin of K24's compose in numpy (``Phy_obj_atk_light(host_chain=True)``): uint8 [H, W, 3] base and one record ->
    the lit uint8 [H, W, 3], float64 / fp32 with the roundings of the reference's chain."""
    h, w, _ = base_hwc.shape
    k, b, beta, full, end, s = (rec[i] for i in range(6))
    d = np.abs(k * np.arange(w, dtype=np.float64)[None, :] - np.arange(h, dtype=np.float64)[:, None] + b) / s
    with np.errstate(divide="ignore", invalid="ignore"):
        att = np.where(d <= full, 1.0, np.where(d <= end, beta / (d * d), 0.0))
    lit = (np.stack([rec[6 + i] * att for i in range(3)], -1) * 255.0).astype(np.float32)
    return np.clip(base_hwc.astype(np.float32) + lit, 0.0, 255.0).astype(np.uint8)


def tube_light_state(n_queries, device):
    """Device state of one tube-light search (K24): (state int32 [2] = (cursor 0, best query -1), best float [1] = 1e10,
    cost float [n_queries] zeros)."""
    if int(n_queries) < 1:
        raise RuntimeError("tube_light_state: need at least one query")
    state = torch.tensor([0, -1], dtype=torch.int32).to(device, non_blocking=True)
    best = torch.full((1,), 1e10, device=device, dtype=torch.float32)
    return state, best, torch.zeros(int(n_queries), device=device, dtype=torch.float32)


def tube_light_compose(table, index, base_u8, out=None):
    """The object lit by the tube light of record ``index[0]`` (a device int32: nothing of the query comes from the host) of
    ``table`` [n, 10] float64: ``base_u8`` [1 or no batch, 3, H, W] uint8 -> fp32 [1, 3, H, W], bit-equal to the reference's
    numpy / OpenCV / PIL chain.  An index outside [0, n) leaves ``out`` as it is."""
    if table.dim() != 2 or table.shape[1] != LIGHT_REC:
        raise RuntimeError("tube_light_compose: table must be [n, %d] float64" % LIGHT_REC)
    if index.dtype != torch.int32 or index.numel() < 1:
        raise RuntimeError("tube_light_compose: index must be int32")
    if base_u8.dtype != torch.uint8 or base_u8.numel() % 3 or base_u8.dim() < 3 or base_u8.shape[-3] != 3 \
            or base_u8.numel() != 3 * base_u8.shape[-2] * base_u8.shape[-1]:
        raise RuntimeError("tube_light_compose: base must be uint8 [3, H, W]")
    H, W = int(base_u8.shape[-2]), int(base_u8.shape[-1])
    if out is None:
        out = torch.zeros((1, 3, H, W), device=base_u8.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or out.numel() != base_u8.numel():
        raise RuntimeError("tube_light_compose: out must be fp32 of the base's size")
    N.check(N.lib().dmh_tube_light_compose(N.ptr_f64(table), N.ptr(index), N.ptr(base_u8), N.ptr(out), int(table.shape[0]), H, W,
                                           N.stream()))
    return out


def tube_light_commit(cost_in, cost, best, state):
    """In place, on the device (phy_obj_atk_light.py:165-167): the query the cursor state[0] points at gets ``cost_in`` (device
    scalar) into ``cost``; a strictly smaller cost than ``best`` becomes the best and its query state[1]; the cursor advances."""
    if cost_in.numel() != 1 or cost_in.dtype != torch.float32 or best.numel() != 1 or best.dtype != torch.float32 \
            or cost.dtype != torch.float32:
        raise RuntimeError("tube_light_commit: cost_in and best must be one fp32 value each, cost fp32")
    if state.dtype != torch.int32 or state.numel() < 2:
        raise RuntimeError("tube_light_commit: state must be int32[2]")
    N.check(N.lib().dmh_tube_light_commit(N.ptr(cost_in), N.ptr(cost), N.ptr(best), N.ptr(state), int(cost.numel()), N.stream()))
    return state


GAUSS_REGION = (90, 170, 100, 200)      # rows 90:170, columns 100:200 of the object (phy_obj_atk_guassian.py:88)


def gauss_sigmas(steps, h, w):
    """Host: the sigmas of a ``steps``-step Gaussian-blur attack on an h x w object, in Python floats as the reference
    accumulates them (phy_obj_atk_guassian.py:76-95): ``epsilon += 1.0 / steps``, ``sigma = epsilon * (max(h, w) // 2)``."""
    if int(steps) < 1:
        raise RuntimeError("gauss_sigmas: need at least one step")
    epsilon, stepsize, max_sigma, out = 0.0, 1.0 / int(steps), max(int(h), int(w)) // 2, []
    for _ in range(int(steps)):
        epsilon += stepsize
        out.append(epsilon * max_sigma)
    return out


def gauss_blur_table(sigmas):
    """Host: (weights float64 [n, max lw + 1], radii int32 [n]) of K26.  Row s holds p[0 .. lw] -- the left half and the centre
    of the symmetric kernel -- of scipy's ``_gaussian_kernel1d`` for sigma s with truncate 4.0, in float64 and in its order:
    lw = int(4.0 * s + 0.5), p = exp(-0.5 / (s * s) * x ** 2) for x = -lw .. lw, p / p.sum(); zero padded."""
    sigmas = [float(s) for s in sigmas]
    if not sigmas:
        raise RuntimeError("gauss_blur_table: need at least one sigma")
    if not all(s > 0.0 and np.isfinite(s) for s in sigmas):
        raise RuntimeError("gauss_blur_table: every sigma must be positive and finite")
    radii = np.asarray([int(4.0 * s + 0.5) for s in sigmas], dtype=np.int32)
    weights = np.zeros((len(sigmas), int(radii.max()) + 1), dtype=np.float64)
    for row, s, lw in zip(weights, sigmas, radii.tolist()):
        x = np.arange(-lw, lw + 1)
        p = np.exp(-0.5 / (s * s) * x ** 2)
        row[:lw + 1] = (p / p.sum())[:lw + 1]
    return weights, radii


def _gauss_region(region, H, W, name):
    """``region`` = (r0, r1, c0, c1) clipped to an H x W patch the way the slices [r0:r1, c0:c1] clip."""
    if len(region) != 4:
        raise RuntimeError("%s: region must be (r0, r1, c0, c1)" % name)
    r0, r1, _ = slice(int(region[0]), int(region[1])).indices(H)
    c0, c1, _ = slice(int(region[2]), int(region[3])).indices(W)
    if r1 <= r0 or c1 <= c0:
        raise RuntimeError("%s: the rectangle %s clips to empty on a %d x %d patch" % (name, tuple(region), H, W))
    return r0, r1, c0, c1


def _gauss_axis_host(a, idx, p, lw):
    """correlate1d of scipy (symmetric branch, mode 'reflect') along the last axis of ``a`` at the positions ``idx``: float64,
    the taps in scipy's order, every operation rounded on its own; the result rounded to fp32."""
    n = a.shape[-1]
    a = a.astype(np.float64)

    def r(j):
        m = np.mod(j, 2 * n)
        return np.where(m >= n, 2 * n - 1 - m, m)
    tmp = a[..., idx] * p[lw]
    for ll in range(-lw, 0):
        tmp = tmp + (a[..., r(idx + ll)] + a[..., r(idx - ll)]) * p[lw + ll]
    return tmp.astype(np.float32)


def gauss_blur_host(x, sigma, region=None):
    """Host twin of K26 in numpy (``Phy_obj_atk_guassian(host_chain=True)``): np.clip(gaussian_filter(x, [0, .., 0, s, s]), 0, 1) of
    fp32 ``x`` [..., H, W] on the rectangle ``region`` (the whole patch by default), bit-equal to scipy's."""
    x = np.asarray(x, dtype=np.float32)
    H, W = x.shape[-2:]
    r0, r1, c0, c1 = _gauss_region((0, H, 0, W) if region is None else region, H, W, "gauss_blur_host")
    weights, radii = gauss_blur_table([sigma])
    p, lw = weights[0], int(radii[0])
    rows = _gauss_axis_host(np.swapaxes(x, -1, -2), np.arange(r0, r1), p, lw)        # axis H first: [..., W, rh]
    out = _gauss_axis_host(np.swapaxes(rows, -1, -2), np.arange(c0, c1), p, lw)      # then axis W: [..., rh, rw]
    return np.clip(out, 0, 1)


def _gauss_obj(obj, name):
    if obj.dtype != torch.float32 or obj.dim() not in (3, 4) or (obj.dim() == 4 and obj.shape[0] != 1):
        raise RuntimeError("%s: obj must be fp32 [1, C, H, W] or [C, H, W]" % name)
    return tuple(int(v) for v in obj.shape[-3:])


def gauss_blur_windows(obj, weights, radii, region=GAUSS_REGION):
    """K26: np.clip(scipy.ndimage.gaussian_filter(obj, [0, 0, s, s]), 0, 1) on the rectangle ``region`` = (r0, r1, c0, c1) of
    fp32 ``obj`` [1, C, H, W] for every row of ``(weights, radii) = gauss_blur_table(sigmas)`` (device float64 [n, k] / int32
    [n]) -> fp32 [n, C, r1 - r0, c1 - c0], bit-equal to scipy's; two launches for all n."""
    C_, H, W = _gauss_obj(obj, "gauss_blur_windows")
    if weights.dim() != 2 or weights.dtype != torch.float64:
        raise RuntimeError("gauss_blur_windows: weights must be float64 [steps, k]")
    n = int(weights.shape[0])
    if n < 1 or int(weights.shape[1]) < 1:
        raise RuntimeError("gauss_blur_windows: need at least one step")
    if radii.dtype != torch.int32 or radii.dim() != 1 or int(radii.shape[0]) != n:
        raise RuntimeError("gauss_blur_windows: radii must be int32 [steps]")
    r0, r1, c0, c1 = _gauss_region(region, H, W, "gauss_blur_windows")
    tmp = torch.empty((n, C_, r1 - r0, W), device=obj.device, dtype=torch.float32)
    windows = torch.empty((n, C_, r1 - r0, c1 - c0), device=obj.device, dtype=torch.float32)
    N.check(N.lib().dmh_gauss_blur_windows(N.ptr(obj), N.ptr_f64(weights), N.ptr(radii), N.ptr(tmp), N.ptr(windows), n,
                                           int(weights.shape[1]), C_, H, W, r0, r1, c0, c1, N.stream()))
    return windows


def gauss_blur_compose(windows, index, obj, region=GAUSS_REGION, out=None):
    """The object with window ``index[0]`` (a device int32: nothing of the step comes from the host) of ``windows``
    [n, C, rh, rw] in the rectangle ``region`` and ``obj`` elsewhere -> fp32 [1, C, H, W].  An index outside [0, n) leaves
    ``out`` as it is."""
    C_, H, W = _gauss_obj(obj, "gauss_blur_compose")
    r0, r1, c0, c1 = _gauss_region(region, H, W, "gauss_blur_compose")
    if windows.dtype != torch.float32 or windows.dim() != 4 or int(windows.shape[0]) < 1 \
            or tuple(windows.shape[1:]) != (C_, r1 - r0, c1 - c0):
        raise RuntimeError("gauss_blur_compose: windows must be fp32 [steps, %d, %d, %d] for this rectangle" % (C_, r1 - r0, c1 - c0))
    if index.dtype != torch.int32 or index.numel() < 1:
        raise RuntimeError("gauss_blur_compose: index must be int32")
    if out is None:
        out = torch.zeros((1, C_, H, W), device=obj.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or out.numel() != obj.numel():
        raise RuntimeError("gauss_blur_compose: out must be fp32 of the object's size")
    N.check(N.lib().dmh_gauss_blur_compose(N.ptr(windows), N.ptr(index), N.ptr(obj), N.ptr(out), int(windows.shape[0]), C_, H, W,
                                           r0, r1, c0, c1, N.stream()))
    return out


def square_sides(n_queries, c, h, w, p_init=0.8, resc_schedule=True):
    """Host: the side of the square of every iteration of a Square attack of ``n_queries`` iterations on a c x h x w object, in
    Python floats as the reference makes it: ``p_selection`` (phy_obj_atk_square.py:222-249, with ``int(it / n_queries *
    10000)`` under ``resc_schedule``) and ``s = max(int(round(sqrt(p * n_features / c))), 1)`` (:281)."""
    import math
    n_queries = int(n_queries)
    if n_queries < 1:
        raise RuntimeError("square_sides: need at least one query")
    n_features, out = c * h * w, []
    for it in range(n_queries):
        if resc_schedule:
            it = int(it / n_queries * 10000)
        p = p_init
        for above, div in ((10, 2), (50, 4), (200, 8), (500, 16), (1000, 32), (2000, 64), (4000, 128), (6000, 256), (8000, 512)):
            if it > above:
                p = p_init / div
        out.append(max(int(round(math.sqrt(p * n_features / c))), 1))
    return out


def square_table(n_queries, c, h, w, p_init=0.8, resc_schedule=True):
    """Host: every draw of a Square attack, from the CPU torch global generator with the reference's expressions in its call
    order -- the start stripes ``sign(2 rand([1, c, 1, w]) - 1)`` (:259-260, :173-175), then per iteration ``vh``, ``vw`` =
    ``(0 + (h - s - 0) rand([1])).long()`` (:177-179, :282-283) and the signs ``sign(2 rand([c, 1, 1]) - 1)`` (:286).
    Returns (table int32 [n_queries + 1, 3 + c] = (vh, vw, s, signs) with row q the square of iteration q - 1 and row 0 zero:
    query 0 is the stripes; stripes fp32 [c, w]).  A side larger than min(h, w) -- where the reference would slice with a negative
    bound -- is refused before any draw."""
    sides = square_sides(n_queries, c, h, w, p_init, resc_schedule)
    if max(sides) > min(h, w):
        raise RuntimeError("square_table: the schedule's largest square (%d) exceeds the %d x %d object; lower p_init"
                           % (max(sides), h, w))
    stripes = torch.sign(2 * torch.rand([1, c, 1, w]) - 1).reshape(c, w).contiguous()
    table = np.zeros((len(sides) + 1, 3 + c), dtype=np.int32)
    for row, s in zip(table[1:], sides):
        vh = (0 + (h - s - 0) * torch.rand([1])).long()
        vw = (0 + (w - s - 0) * torch.rand([1])).long()
        sign = torch.sign(2 * torch.rand([c, 1, 1]) - 1)
        row[0], row[1], row[2] = int(vh), int(vw), s
        row[3:] = sign.reshape(c).numpy()
    return table, stripes


def _square_operands(name, x0, x_best, x_new, table, stripes):
    if x0.dtype != torch.float32 or x0.dim() not in (3, 4) or (x0.dim() == 4 and x0.shape[0] != 1):
        raise RuntimeError("%s: x0 must be fp32 [1, C, H, W] or [C, H, W]" % name)
    C_, H, W = (int(v) for v in x0.shape[-3:])
    for t in (x_best, x_new):
        if t.dtype != torch.float32 or t.numel() != x0.numel() or tuple(t.shape[-3:]) != (C_, H, W):
            raise RuntimeError("%s: x_best and x_new must be fp32 of x0's size" % name)
    ptrs = {x0.data_ptr(), x_best.data_ptr(), x_new.data_ptr()}
    if len(ptrs) != 3:
        raise RuntimeError("%s: x0, x_best and x_new must be three different buffers" % name)
    if table.dtype != torch.int32 or table.dim() != 2 or int(table.shape[0]) < 1 or int(table.shape[1]) != 3 + C_:
        raise RuntimeError("%s: table must be int32 [n, %d]" % (name, 3 + C_))
    if stripes.dtype != torch.float32 or tuple(stripes.shape) != (C_, W):
        raise RuntimeError("%s: stripes must be fp32 [%d, %d]" % (name, C_, W))
    return C_, H, W


def square_propose(x0, x_best, x_new, table, stripes, state, eps):
    """K27, in place, driven by K24's ``state`` = (cursor q, best query) on the device: if query q - 1 became the best,
    ``x_best`` <- ``x_new``; then ``x_new`` <- the candidate of query q -- the stripes for q = 0, else ``x_best`` with the square
    of ``table`` row q pushed by 2 eps sign_c and projected onto [x0 - eps, x0 + eps] and [0, 1] (phy_obj_atk_square.py:284-291),
    bit-equal to the torch expression.  q = n only absorbs; any other q outside [0, n) does nothing."""
    C_, H, W = _square_operands("square_propose", x0, x_best, x_new, table, stripes)
    if state.dtype != torch.int32 or state.numel() < 2:
        raise RuntimeError("square_propose: state must be int32[2]")
    if not float(eps) >= 0.0:
        raise RuntimeError("square_propose: eps must not be negative")
    N.check(N.lib().dmh_square_propose(N.ptr(x0), N.ptr(x_best), N.ptr(x_new), N.ptr(table), N.ptr(stripes), N.ptr(state),
                                       int(table.shape[0]), C_, H, W, float(eps), N.stream()))
    return x_new


def square_host(x0, x_best, x_new, table, stripes, q, accept, eps):
    """Host twin of K27 in torch on the CPU (``Phy_obj_atk_Square(host_chain=True)``): returns the new (x_best, x_new) for query
    ``q`` after the decision ``accept`` about query q - 1, with the reference's own expressions (:259-260, :284-291)."""
    C_, H, W = _square_operands("square_host", x0, x_best, x_new, torch.as_tensor(table), stripes)
    n = len(table)
    if accept and 0 < q <= n:
        x_best = x_new.clone()
    if q == 0:
        x_new = torch.clamp(x0 + eps * stripes.reshape(1, C_, 1, W), 0., 1.).reshape(x0.shape)
    elif 0 < q < n:
        vh, vw, s = (int(v) for v in table[q][:3])
        new_deltas = torch.zeros([C_, H, W])
        new_deltas[:, vh:vh + s, vw:vw + s] = 2. * eps * torch.as_tensor(table[q][3:]).float().reshape(C_, 1, 1)
        x_new = x_best.reshape(C_, H, W) + new_deltas
        x_new = torch.min(torch.max(x_new, x0.reshape(C_, H, W) - eps), x0.reshape(C_, H, W) + eps)
        x_new = torch.clamp(x_new, 0., 1.).reshape(x0.shape)
    return x_best, x_new


def l0_compose_fwd_launch(obj, pos, neg, l0_clip, finalize):
    """K5 on contiguous tensors: (adv, count int32 [1])."""
    if obj.dim() != 4 or obj.shape[0] != 1 or obj.shape != pos.shape or obj.shape != neg.shape:
        raise RuntimeError("l0_compose: obj/pos/neg must all be [1,C,H,W]")
    adv = torch.empty_like(obj)
    count = torch.zeros(1, device=obj.device, dtype=torch.int32)
    N.check(N.lib().dmh_l0_compose_fwd(N.ptr(obj), N.ptr(pos), N.ptr(neg), obj.shape[1], obj.shape[2] * obj.shape[3],
                                       float(l0_clip), int(finalize), N.ptr(adv), N.ptr(count), N.stream()))
    return adv, count


def l0_compose_bwd_launch(obj, pos, neg, g_adv):
    g_pos, g_neg = torch.empty_like(pos), torch.empty_like(neg)
    N.check(N.lib().dmh_l0_compose_bwd(N.ptr(obj), N.ptr(pos), N.ptr(neg), N.ptr(g_adv), obj.shape[1], obj.shape[2] * obj.shape[3],
                                       N.ptr(g_pos), N.ptr(g_neg), 0, N.stream()))
    return g_pos, g_neg


class _L0Compose(torch.autograd.Function):
    @staticmethod
    def forward(ctx, obj, pos, neg, l0_clip, finalize):
        adv, count = l0_compose_fwd_launch(obj, pos, neg, l0_clip, finalize)
        ctx.save_for_backward(obj, pos, neg)
        ctx.mark_non_differentiable(count)
        return adv, count

    @staticmethod
    def backward(ctx, g_adv, g_count):
        obj, pos, neg = ctx.saved_tensors
        g_pos, g_neg = l0_compose_bwd_launch(obj, pos, neg, _c(g_adv))
        return None, g_pos, g_neg, None, None


def l0_compose(obj, pos, neg, l0_clip=1.0 / 255.0, finalize=False):
    """adv = clamp(obj + clamp(pos,0,1) - clamp(neg,0,1), 0, 1) and the L0 count of the thresholded
    pattern (phy_obj_atk_l0.py:94-99, 43-52; finalize=True applies :143-150).  Returns (adv, count[int32,1])."""
    return _L0Compose.apply(_c(obj), _c(pos), _c(neg), float(l0_clip), bool(finalize))


def l0_mask_cost_fwd_launch(pos, neg):
    if pos.dim() != 4 or pos.shape[0] != 1 or pos.shape != neg.shape:
        raise RuntimeError("l0_mask_cost: pos/neg must be [1,C,H,W]")
    lib = N.lib()
    Cc, HW = pos.shape[1], pos.shape[2] * pos.shape[3]
    part = torch.empty(lib.dmh_l0_mask_partials_size(HW), device=pos.device, dtype=torch.float32)
    cost = torch.empty((), device=pos.device, dtype=torch.float32)
    N.check(lib.dmh_l0_mask_cost_fwd(N.ptr(pos), N.ptr(neg), Cc, HW, N.ptr(part), N.ptr(cost), N.stream()))
    return cost


def l0_mask_cost_bwd_launch(pos, neg, g):
    g_pos, g_neg = torch.empty_like(pos), torch.empty_like(neg)
    N.check(N.lib().dmh_l0_mask_cost_bwd(N.ptr(pos), N.ptr(neg), pos.shape[1], pos.shape[2] * pos.shape[3],
                                         N.ptr(_c(g.to(torch.float32))), None, N.ptr(g_pos), N.ptr(g_neg), 0, N.stream()))
    return g_pos, g_neg


class _L0MaskCost(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, neg):
        ctx.save_for_backward(pos, neg)
        return l0_mask_cost_fwd_launch(pos, neg)

    @staticmethod
    def backward(ctx, g):
        return l0_mask_cost_bwd_launch(*ctx.saved_tensors, g)


def l0_mask_cost(pos, neg):
    """mean(max_c(tanh(pos/10)/(2-1e-7)+0.5)) + same for neg (phy_obj_atk_l0.py:130-132)."""
    return _L0MaskCost.apply(_c(pos), _c(neg))


L0_REC = 8          # floats per record of the fused L0 update (DMH_L0_REC)
L0_BETAS = (0.5, 0.9)   # phy_obj_atk_l0.py:85; K23 holds them as constants


def l0_adam_table(steps, lr):
    """Adam's bias corrections for t = 1 .. 2 * steps as K23 reads them: a host fp32 tensor [2 * steps, 2] of
    (lr / (1 - b1^t), sqrt(1 - b2^t)), computed in double and rounded once."""
    import math
    b1, b2 = L0_BETAS
    rows = [(float(lr) / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)) for t in range(1, 2 * int(steps) + 1)]
    return torch.tensor(rows, dtype=torch.float64).to(torch.float32)


class L0FusedState(object):
    """The device buffers of one fused L0 attack of ``steps`` (2 * steps iterations at the most): the two patterns (taken over,
    updated in place), Adam's m / v for both, the composed patch, and the controller's words -- count int32 [2 steps + 1], rec
    [2 steps, L0_REC], cursor int32 [2], tab [2 steps, 2].  Nothing here is read by the host while the attack runs."""

    def __init__(self, pos, neg, steps, lr):
        steps = int(steps)
        if steps < 1 or steps >= 1 << 24:
            raise RuntimeError("L0FusedState: steps must lie in [1, 2^24)")
        _need_cuda(pos)
        dev = pos.device
        self.steps = steps
        self.pos, self.neg = _c(pos.detach()), _c(neg.detach())
        state = torch.zeros((4,) + tuple(pos.shape), device=dev, dtype=torch.float32)
        self.m_pos, self.v_pos, self.m_neg, self.v_neg = state[0], state[1], state[2], state[3]
        self.adv = torch.empty_like(self.pos)
        self.count = torch.zeros(2 * steps + 1, device=dev, dtype=torch.int32)
        self.rec = torch.zeros((2 * steps, L0_REC), device=dev, dtype=torch.float32)
        self.cursor = torch.zeros(2, device=dev, dtype=torch.int32)
        self.tab = l0_adam_table(steps, lr).to(dev, non_blocking=True)

    def step(self, obj, g_adv, adv_cost, mask_cost, mask_wt, thresh, l0_clip):
        return l0_fused_step(obj, self.pos, self.neg, self.m_pos, self.v_pos, self.m_neg, self.v_neg, g_adv, self.adv,
                             self.count, self.rec, self.cursor, self.tab, adv_cost, mask_cost, self.steps, mask_wt, thresh,
                             l0_clip)


def l0_fused_step(obj, pos, neg, m_pos, v_pos, m_neg, v_neg, g_adv, adv, count, rec, cursor, tab, adv_cost, mask_cost, steps,
                  mask_wt, thresh, l0_clip=1.0 / 255.0):
    """K23, in place: iteration i = cursor[0] of the L0 attack from ``g_adv`` = d adv_cost / d composed patch to the next composed
    patch ``adv`` -- mask weight from count[i] / count[0] <= thresh, both clamps' gates, the mask cost's gradient, Adam on both
    patterns, compose, count[i + 1], record i, cursor + 1 (phy_obj_atk_l0.py:92-138).  No host value of the iteration enters."""
    steps = int(steps)
    if obj.dim() != 4 or obj.shape[0] != 1:
        raise RuntimeError("l0_fused_step: obj must be [1,C,H,W]")
    n = obj.numel()
    for t in (obj, pos, neg, m_pos, v_pos, m_neg, v_neg, g_adv, adv):
        if t.numel() != n or t.dtype != torch.float32:
            raise RuntimeError("l0_fused_step: the patch-sized tensors must be fp32 and of one size")
    if steps < 1 or steps >= 1 << 24:
        raise RuntimeError("l0_fused_step: steps must lie in [1, 2^24)")
    if count.dtype != torch.int32 or count.numel() < 2 * steps + 1:
        raise RuntimeError("l0_fused_step: count must be int32[2 * steps + 1]")
    if rec.dtype != torch.float32 or rec.numel() < 2 * steps * L0_REC:
        raise RuntimeError("l0_fused_step: rec must hold 2 * steps records of %d floats" % L0_REC)
    if tab.dtype != torch.float32 or tab.numel() < 4 * steps:
        raise RuntimeError("l0_fused_step: tab must hold 2 * steps pairs of floats")
    if cursor.dtype != torch.int32 or cursor.numel() < 2:
        raise RuntimeError("l0_fused_step: cursor must be int32[2]")
    for name, t in (("adv_cost", adv_cost), ("mask_cost", mask_cost)):
        if t is not None and (t.numel() != 1 or t.dtype != torch.float32):
            raise RuntimeError("l0_fused_step: %s must be one fp32 value" % name)
    N.check(N.lib().dmh_l0_fused_step(N.ptr(obj), N.ptr(pos), N.ptr(neg), N.ptr(m_pos), N.ptr(v_pos), N.ptr(m_neg), N.ptr(v_neg),
                                      N.ptr(g_adv), N.ptr(adv), N.ptr(count), N.ptr(rec), N.ptr(cursor), N.ptr(tab),
                                      N.ptr(adv_cost), N.ptr(mask_cost), steps, obj.shape[1], obj.shape[2] * obj.shape[3],
                                      float(mask_wt), float(thresh), float(l0_clip), N.stream()))
    return adv
