"""K3 (csrc/eot_paste.hip) in plain float64 numpy, written from its definition -- not from the kernel:

    adv[n]      = flip_n( resize( scene_n (1 - mk_n) + o_n mk_n ) )         (warp-only mode: resize(o_n))
    mask_out[n] = flip_n( resize( mk_n ) )
    o_n, mk_n   = bilinear_zeros( pad(patch | mask), S_n(X + 0.5, Y + 0.5) - 0.5 )
    S_n(x, y)   = ((c0 x + c1 y + c2) / (c6 x + c7 y + 1), (c3 x + c4 y + c5) / (c6 x + c7 y + 1))

(torchvision 0.8.2's Pad / perspective / Resize, oracle/tv082.py).  ``flip`` mirrors the FINISHED sample; ``scene_index`` picks
the frame of a pool; a scene with one frame is broadcast.  The adjoint with respect to the patch goes by SCATTER through the
forward's own index map (np.add.at) where the kernel gathers per texel over the inverse homography.  Every function can return
the same operation on absolute values (a - b becomes |a| + |b|): the S of tests/util.py: round_bound_violations.

tests/test_paste_ref.py pins this file on the float64 torch chain of oracle/tv082.py and checks the input conditions of the
cases below; tests/test_gpu_paste_anchor.py holds the kernels to it.
"""
import numpy as np

COMPOSITE, WARP_ONLY = 0, 1
TILED, FOUR_WIDE, GENERIC = 2, 1, 0         # dmh_eot_paste_fwd_form
LPT = 16                                    # csrc/eot_paste.hip: lanes per texel of the backward (sample n goes to lane n % LPT)


# ---- the index map ------------------------------------------------------------------------------------------------------------

def sample_coords(coeffs, SH, SW):
    """Sample coordinates (x, y) [N, SH, SW] in the padded frame, float64: S_n at the pixel centres, less the half pixel."""
    c = np.asarray(coeffs, np.float64).reshape(-1, 8)[:, :, None, None]
    xn, yn = np.arange(SW, dtype=np.float64)[None, None, :] + 0.5, np.arange(SH, dtype=np.float64)[None, :, None] + 0.5
    den = c[:, 6] * xn + c[:, 7] * yn + 1.0
    return (c[:, 0] * xn + c[:, 1] * yn + c[:, 2]) / den - 0.5, (c[:, 3] * xn + c[:, 4] * yn + c[:, 5]) / den - 0.5


def sample_coords_fp32(coeffs, SH, SW):
    """The fp32 transcription of torchvision's coordinate chain (c / (0.5 SW), numerator, / den - 1, ((g + 1) SW - 1) / 2), one
    rounding per operation.  Where it equals sample_coords at every pixel, an fp32 implementation has no coordinate error at all."""
    f = np.float32
    c = np.asarray(coeffs, np.float64).reshape(-1, 8).astype(f)[:, :, None, None]
    sx, sy = f(0.5) * f(SW), f(0.5) * f(SH)
    xn, yn = np.arange(SW, dtype=f)[None, None, :] + f(0.5), np.arange(SH, dtype=f)[None, :, None] + f(0.5)
    den = xn * c[:, 6] + yn * c[:, 7] + f(1)
    gx = (xn * (c[:, 0] / sx) + yn * (c[:, 1] / sx) + c[:, 2] / sx) / den - f(1)
    gy = (xn * (c[:, 3] / sy) + yn * (c[:, 4] / sy) + c[:, 5] / sy) / den - f(1)
    x, y = ((gx + f(1)) * f(SW) - f(1)) / f(2), ((gy + f(1)) * f(SH) - f(1)) / f(2)
    assert x.dtype == f and y.dtype == f
    return x, y


def index_map(coeffs, SH, SW, PH, PW, l_pad, t_pad):
    """The four bilinear taps of every composite pixel: (texel [N, SH*SW, 4] as v * PW + u, or -1 outside the patch rectangle --
    the zero padding --, weight [N, SH*SW, 4] float64).  Tap order: (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1)."""
    x, y = sample_coords(coeffs, SH, SW)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    N = x.shape[0]
    tex, w = np.empty((N, SH * SW, 4), np.int64), np.empty((N, SH * SW, 4), np.float64)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        u, v = x0 + dx - l_pad, y0 + dy - t_pad
        inside = (u >= 0) & (u < PW) & (v >= 0) & (v < PH)
        tex[:, :, k] = np.where(inside, v * PW + u, -1).reshape(N, -1)
        w[:, :, k] = ((fx if dx else 1.0 - fx) * (fy if dy else 1.0 - fy)).reshape(N, -1)
    return tex, w


def bilinear_zeros(planes, taps):
    """planes [C, PH, PW] sampled through the index map: [N, C, SH*SW]."""
    tex, w = taps
    flat = np.asarray(planes, np.float64).reshape(planes.shape[0], -1)
    vals = np.where(tex[:, None] >= 0, flat[:, np.maximum(tex, 0)].transpose(1, 0, 2, 3), 0.0)       # [N, C, P, 4]
    return (vals * w[:, None]).sum(-1)


def resize_matrix(S, O, weights="float64"):
    """F.interpolate(bilinear, align_corners=False) along one axis as a dense [O, S] matrix: output o reads i0 = floor(src) with
    1 - l and min(i0 + 1, S - 1) with l, src = max(r (o + 0.5) - 0.5, 0), r = S / O.  ``weights``: 'float64', or 'fp32' -- r, src,
    i0 and l formed in np.float32 as ATen's fp32 kernel forms them, everything after that float64."""
    o = np.arange(O)
    if weights == "fp32":
        f = np.float32
        r = f(S) / f(O)
        # r (o + 0.5) - 0.5 as ONE fused multiply-add, which is what ATen's CPU kernel and hipcc's contraction of the kernel's
        # expression both evaluate: the product of a 24-bit and an 11-bit number is exact in float64, the sum too, then one
        # rounding.  (With a rounded product the coordinate differs by an ulp at 1 of 63 columns of 64 -> 63: test_paste_ref.py
        # holds this form, not that one, to fp32 F.interpolate.)
        src = np.maximum((np.float64(r) * (o + 0.5) - 0.5).astype(f), f(0))
        assert src.dtype == f and O + 1 < 2 ** 11
        i0 = src.astype(np.int64)
        lam = (src - i0.astype(f)).astype(np.float64)
    else:
        assert weights == "float64", weights
        src = np.maximum((float(S) / float(O)) * (o + 0.5) - 0.5, 0.0)
        i0 = np.floor(src).astype(np.int64)
        lam = src - i0
    i1 = np.minimum(i0 + 1, S - 1)
    R = np.zeros((O, S), np.float64)
    np.add.at(R, (o, i0), 1.0 - lam)
    np.add.at(R, (o, i1), lam)
    return R


# ---- forward and adjoint ----------------------------------------------------------------------------------------------------------

class Paste(object):
    """One geometry: the index map and the resize matrices, formed once and shared by every variant of a case."""

    def __init__(self, coeffs, frame, patch_hw, pad_lt, out, weights="float64", taps=None):
        (self.SH, self.SW), (self.PH, self.PW), (self.l_pad, self.t_pad), (self.OH, self.OW) = frame, patch_hw, pad_lt, out
        self.coeffs = np.asarray(coeffs, np.float64).reshape(-1, 8)
        self.N = self.coeffs.shape[0]
        self.taps = index_map(self.coeffs, self.SH, self.SW, self.PH, self.PW, self.l_pad, self.t_pad) if taps is None else taps
        self.Ry, self.Rx = resize_matrix(self.SH, self.OH, weights), resize_matrix(self.SW, self.OW, weights)

    def _resize(self, planes):      # [..., SH*SW] -> [..., OH, OW]
        p = planes.reshape(planes.shape[:-1] + (self.SH, self.SW))
        return np.matmul(np.matmul(self.Ry, p), self.Rx.T)

    def _flip(self, out, flip):
        if flip is None:
            return out
        out = out.copy()
        for n in np.nonzero(np.asarray(flip))[0]:
            out[n] = out[n][..., ::-1]
        return out

    def forward(self, scene, patch, mask, mode=COMPOSITE, flip=None, scene_index=None, absolute=False):
        """(adv [N, 3, OH, OW], mask_out [N, 1, OH, OW]) in float64.  scene [P, 3, SH, SW] (ignored in warp-only mode): P = 1 is
        broadcast, P = N is per sample, a pool goes with scene_index [N].  ``absolute``: the operation on absolute values."""
        patch, mask = np.asarray(patch, np.float64).reshape(3, self.PH, self.PW), np.asarray(mask, np.float64).reshape(1, self.PH, self.PW)
        if absolute:
            patch, mask = np.abs(patch), np.abs(mask)
        o, mk = bilinear_zeros(patch, self.taps), bilinear_zeros(mask, self.taps)
        if mode == WARP_ONLY:
            comp = o
        else:
            scene = np.asarray(scene, np.float64)
            idx = np.asarray(scene_index) if scene_index is not None else (np.zeros(self.N, int) if scene.shape[0] == 1 else np.arange(self.N))
            assert scene_index is not None or scene.shape[0] in (1, self.N)
            sc = scene[idx].reshape(self.N, 3, -1)
            comp = np.abs(sc) * (1.0 + mk) + o * mk if absolute else sc * (1.0 - mk) + o * mk
        return self._flip(self._resize(comp), flip), self._flip(self._resize(mk), flip)

    def backward(self, g_adv, mask, mode=COMPOSITE, flip=None, absolute=False, skip_samples=()):
        """d <g_adv, adv> / d patch [3, PH, PW] in float64, by scatter: the mirrored g_adv back through the resize, times mk, and
        every composite pixel adds weight x that to its four texels.  ``skip_samples``: samples left out (a mutation for the tests)."""
        g = self._flip(np.asarray(g_adv, np.float64), flip)
        mask = np.asarray(mask, np.float64).reshape(1, self.PH, self.PW)
        if absolute:
            g, mask = np.abs(g), np.abs(mask)
        g_comp = np.matmul(np.matmul(self.Ry.T, g), self.Rx).reshape(self.N, 3, -1)       # the resize's transpose
        if mode != WARP_ONLY:
            g_comp = g_comp * bilinear_zeros(mask, self.taps)
        tex, w = self.taps
        out = np.zeros((3, self.PH * self.PW), np.float64)
        for n in range(self.N):
            if n in skip_samples:
                continue
            hit = tex[n] >= 0
            for c in range(3):
                np.add.at(out[c], tex[n][hit], (w[n] * g_comp[n, c][:, None])[hit])
        return out.reshape(3, self.PH, self.PW)

    # ---- chain lengths of the kernels' sums, from the index map (never from a kernel's output)

    def reads(self, mask=None):
        """[N, PH*PW]: how many composite pixels of sample n read the texel with a nonzero weight (times a nonzero mk, when a mask
        is given: the composite's gradient passes through mk)."""
        tex, w = self.taps
        live = (tex >= 0) & (w != 0)
        if mask is not None:
            live &= (bilinear_zeros(np.asarray(mask, np.float64).reshape(1, self.PH, self.PW), self.taps)[:, 0] != 0)[:, :, None]
        cnt = np.zeros((self.N, self.PH * self.PW), np.int64)
        for n in range(self.N):
            np.add.at(cnt[n], tex[n][live[n]], 1)
        return cnt

    def resize_taps_per_pixel(self):
        """The largest number of output pixels that read one scene pixel."""
        return int((self.Ry != 0).sum(0).max()) * int((self.Rx != 0).sum(0).max())


def object_extent(coeffs, frame, patch_hw, pad_lt):
    """Per sample, the composite pixels with a nonzero footprint in the patch rectangle: (ymin, ymax, xmin, xmax), or None."""
    tex, w = index_map(coeffs, frame[0], frame[1], patch_hw[0], patch_hw[1], pad_lt[0], pad_lt[1])
    out = []
    for n in range(tex.shape[0]):
        hit = ((tex[n] >= 0) & (w[n] != 0)).any(-1).reshape(frame)
        ys, xs = np.nonzero(hit)
        out.append((ys.min(), ys.max(), xs.min(), xs.max()) if len(ys) else None)
    return out


# ---- n_round, as formulas of the kernels' operations (tests/test_gpu_paste_anchor.py derives them line by line) ------------------

N_SAMPLE = 7            # patch_sample: 1 - fx and 1 - fy (2), their product (1), the tap's product (1), three additions (3)
N_RESIZE = 6            # 1 - lx (1), hx * comp (1), the row's sum (1), 1 - ly (1), hy * (..) (1), the sum (1)
N_FWD_COMPOSITE = 2 * N_SAMPLE + 2 + N_RESIZE       # o * mk: both factors' roundings + the product (1) + the composite's sum (1)
N_FWD_WARP = N_SAMPLE + N_RESIZE                    # warp-only adv, and mask_out in both modes


def n_bwd(P, mode, mask):
    """paste_bwd_kernel: wyy and wxx (1 - l and the sum of the two matches: 2 each) and their product ww (1): 5; the fmaf chain
    into G over the resize taps of one scene pixel: T; wu wv (1 - f: 1 each, product 1): 3; in composite mode times
    patch_sample(mask) (N_SAMPLE + 1); the fmaf chain into acc over candidates x ceil(N / LPT) samples; 4 butterfly additions."""
    K = int(P.reads(mask if mode == COMPOSITE else None).max())
    return 5 + P.resize_taps_per_pixel() + 3 + (N_SAMPLE + 1 if mode == COMPOSITE else 0) + K * -(-P.N // LPT) + 4


# ---- the exact-coordinate cases (a) --------------------------------------------------------------------------------------------------

FRAME_A, FRAME_B = (32, 64), (64, 256)
PATCHES = {"p11x15": ((11, 15), (24, 10)), "p12x16": ((12, 16), (24, 10)), "p20x28": ((20, 28), (100, 20))}     # (PH, PW), (l_pad, t_pad)

# g = h = 0, every entry dyadic: with power-of-two frames the fp32 coordinate chain is exact (test_paste_ref.py checks each)
SETS = {
    # patches at (24, 10): either frame
    "shear": [0.75, 0.125, 3.375, -0.25, 1.25, 2.625],
    "mini": [1.5, 0, -20.25, 0, 1.5, -7.875],
    "magl": [0.375, -0.125, 30.5, 0.0625, 0.5, 9.125],          # magnified 2.7x, over the left edge
    "trans": [1, 0, -3.25, 0, 1, 1.625],                        # a pure fractional translation
    "s25": [2.5, 0, -56.125, 0, 2.5, -27.375],                  # scale 2.5: texels no pixel reads
    "top": [1, 0, 2.5, 0, 1, 14.25],                            # over the top edge
    "rightA": [1, 0, -30.5, 0, 1, -2.75],                       # over the right edge of the 64-wide frame
    "bottomA": [1, 0, 5.25, 0, 1, -15.75],                      # over the bottom edge of the 32-high frame
    # the 20 x 28 patch at (100, 20) in the 64 x 256 frame: across output column 128 and rows 24 / 32
    "seamB": [1, 0, -14.5, 0, 1, 0.375],
    "shearB": [0.75, 0.125, 2.375, -0.25, 1.25, 30.625],
    "miniB": [1.5, 0, -70.25, 0, 1.5, -17.875],
    "maglB": [0.375, -0.125, 101.5, 0.0625, 0.5, 14.125],
    "s25B": [2.5, 0, -221.125, 0, 2.5, -57.375],
    "topB": [1, 0, 20.75, 0, 1, 27.5],
    "rightB": [1, 0, -140.5, 0, 1, 3.25],
    "bottomB": [1, 0, -30.25, 0, 1, -30.75],
}
SETS_A = ("shear", "mini", "magl", "trans", "s25", "top", "rightA", "bottomA")
SETS_B = ("seamB", "shearB", "miniB", "maglB", "s25B", "topB", "rightB", "bottomB")


def coeffs_of(names, cycle=(1.25, -0.625)):
    """[len(names), 8] float64.  A name may come more than once: its k-th repeat is translated by k x ``cycle`` (dyadic)."""
    seen, rows = {}, []
    for nm in names:
        k = seen.get(nm, 0)
        seen[nm] = k + 1
        c = list(SETS[nm]) + [0.0, 0.0]
        c[2] += k * cycle[0]
        c[5] += k * cycle[1]
        rows.append(c)
    return np.array(rows, np.float64)


def cycle_names(sets, N):
    return tuple(sets[i % len(sets)] for i in range(N))


# forward: (id, frame, patch, out, form, misalign adv, resize weights, mask kind, sets)
FWD_CASES = [
    ("A-32x64-tiled", FRAME_A, "p11x15", (32, 64), TILED, False, "float64", "ones", SETS_A),
    ("A-64x128-tiled-up", FRAME_A, "p12x16", (64, 128), TILED, False, "float64", "uniform", SETS_A),
    ("B-64x256-tiled", FRAME_B, "p20x28", (64, 256), TILED, False, "float64", "uniform", SETS_B),
    ("B-60x220-tiled-ragged", FRAME_B, "p20x28", (60, 220), TILED, False, "fp32", "ones", SETS_B),
    # 256 / 192 = 1.33 columns per output column: 172 for a tile of 128, more than the 160 the tiled kernel's LDS rectangle holds
    ("B-60x192-fourwide-ragged", FRAME_B, "p20x28", (60, 192), FOUR_WIDE, False, "fp32", "uniform", SETS_B),
    ("A-16x32-fourwide", FRAME_A, "p12x16", (16, 32), FOUR_WIDE, False, "float64", "ones", SETS_A),
    ("A-32x63-generic", FRAME_A, "p11x15", (32, 63), GENERIC, False, "fp32", "uniform", SETS_A),
    ("A-32x64-generic-misaligned", FRAME_A, "p12x16", (32, 64), GENERIC, True, "float64", "uniform", SETS_A),
]

# backward: (id, frame, patch, out, resize weights, mask kind, sample names)
BWD_CASES = [
    ("A-N1-s25", FRAME_A, "p12x16", (32, 64), "float64", "ones", ("s25",)),
    ("A-N1-magl", FRAME_A, "p11x15", (16, 32), "float64", "uniform", ("magl",)),
    ("A-N3", FRAME_A, "p12x16", (32, 63), "fp32", "uniform", ("shear", "rightA", "bottomA")),
    ("A-N16-up", FRAME_A, "p11x15", (64, 128), "float64", "ones", cycle_names(SETS_A, 16)),
    ("A-N17", FRAME_A, "p12x16", (32, 64), "float64", "ones", cycle_names(SETS_A, 17)),
    ("B-N3", FRAME_B, "p20x28", (64, 256), "float64", "uniform", ("seamB", "topB", "maglB")),
    ("B-N33-ragged", FRAME_B, "p20x28", (60, 192), "fp32", "uniform", cycle_names(SETS_B, 33)),
]
FULL_COVERAGE = ("A-N16-up", "A-N17", "B-N33-ragged")        # every texel is read by some sample
SCENE_POOL = (2, 0, 2, 1)                                    # scene_index of a pool of 3 frames, repeated over the samples


def flips_of(N, first=1):
    """Every other sample mirrored, starting with a mirrored one."""
    return np.array([(i + first) % 2 for i in range(N)], np.int32)


def case_inputs(case_id, frame, patch, N, mask_kind, out):
    """fp32 inputs of a case, values uniform in [0, 1] (mask: ones, or uniform in (0, 1]); g_adv uniform in [-0.5, 0.5)."""
    import zlib
    rng = np.random.RandomState(zlib.crc32(case_id.encode()) % (2 ** 31))
    (PH, PW), _ = PATCHES[patch]
    d = {"patch": rng.uniform(0, 1, (1, 3, PH, PW)).astype(np.float32),
         "mask": np.ones((1, 1, PH, PW), np.float32) if mask_kind == "ones" else (1.0 - rng.uniform(0, 1, (1, 1, PH, PW))).astype(np.float32),
         "scenes": rng.uniform(0, 1, (N, 3) + frame).astype(np.float32),
         "pool": rng.uniform(0, 1, (3, 3) + frame).astype(np.float32),
         "g_adv": (rng.uniform(0, 1, (N, 3) + out) - 0.5).astype(np.float32)}
    assert d["mask"].min() > 0
    return d


def edges_crossed(ext, frame):
    """Which frame edges an object_extent touches."""
    if ext is None:
        return set()
    y0, y1, x0, x1 = ext
    return {e for e, hit in (("top", y0 == 0), ("bottom", y1 == frame[0] - 1), ("left", x0 == 0), ("right", x1 == frame[1] - 1)) if hit}


# ---- the perspective cases (b): the float64 chain of oracle/tv082.py, and the same chain in fp32 ----------------------------------

PERSP_SMALL = {"frame": (40, 64), "patch": (12, 16), "pad": (24, 10),
               "outs": [(32, 64), (30, 52), (24, 36), (33, 53), (48, 96)],
               "quads": [[[22, 12], [50, 9], [53, 33], [20, 30]],          # mild trapezoid
                         [[-6, 5], [14, 2], [16, 30], [-4, 26]],           # over the left edge
                         [[30, 20], [70, 14], [75, 47], [28, 39]],         # magnified 2.5x over the lower right corner
                         [[40, 15], [47, 16], [47, 22], [40, 21]]]}        # minified to about 7 x 6 pixels
PERSP_LARGE = {"frame": (96, 320), "patch": (20, 28), "pad": (150, 40),
               "outs": [(80, 256), (84, 200)],
               "quads": [[[140, 30], [200, 35], [195, 80], [150, 70]],     # across output column 128 of (80, 256)
                         [[296, 58], [328, 62], [330, 98], [297, 99]],     # over the right and bottom edges
                         [[20, 10], [52, 12], [50, 34], [22, 30]],
                         [[-8, 50], [30, 44], [34, 90], [-5, 84]]]}        # over the left edge
PERSP_CASES = [(g, out) for g in ("small", "large") for out in (PERSP_SMALL if g == "small" else PERSP_LARGE)["outs"]]


def persp_geometry(name):
    return PERSP_SMALL if name == "small" else PERSP_LARGE


def persp_coeffs(geo, N):
    """N coefficient rows solved by tv082.get_perspective_coeffs (fp32 values): the quads in turn, the k-th round of them moved by
    (3 k, 2 k) pixels."""
    from oracle import tv082
    (PH, PW), (l, t) = geo["patch"], geo["pad"]
    start = [[l, t], [l + PW, t], [l + PW, t + PH], [l, t + PH]]
    rows = []
    for i in range(N):
        k = i // len(geo["quads"])
        q = [[float(p[0] + 3 * k), float(p[1] + 2 * k)] for p in geo["quads"][i % len(geo["quads"])]]
        rows.append(tv082.get_perspective_coeffs([list(map(float, p)) for p in start], q))
    return np.array(rows, np.float64)


def oracle_chain(dtype, scene, patch, mask, coeffs, pad_lt, out, g_adv=None, warp_only=False):
    """tv082.pad -> perspective_coeffs -> composite -> tv082.resize in torch at ``dtype`` on the CPU, and the autograd gradient of
    <g_adv, adv> with respect to the patch: (adv, mask_out, g_patch or None)."""
    import torch
    from oracle import tv082
    scene, patch, mask = (torch.as_tensor(np.asarray(a)).to(dtype) for a in (scene, patch, mask))
    SH, SW = scene.shape[-2:]
    PH, PW = patch.shape[-2:]
    l, t = pad_lt
    p = patch.clone().requires_grad_(True)
    box = [l, t, SW - PW - l, SH - PH - t]
    pp, mp = tv082.pad(p, box), tv082.pad(mask, box)
    advs, ms = [], []
    for n, c in enumerate(np.asarray(coeffs, np.float64)):
        o, mk = tv082.perspective_coeffs(pp, list(c)), tv082.perspective_coeffs(mp, list(c))
        advs.append(o if warp_only else scene[n % scene.shape[0]][None] * (1 - mk) + o * mk)
        ms.append(mk)
    adv, mo = torch.cat(advs), torch.cat(ms)
    if not warp_only:
        adv, mo = tv082.resize(adv, out), tv082.resize(mo, out)
    g = None
    if g_adv is not None:
        (adv * torch.as_tensor(np.asarray(g_adv)).to(dtype)).sum().backward()
        g = p.grad.detach()
    return adv.detach(), mo.detach(), g


# ---- references of the exact cases, built once and shared read-only by the CPU and the GPU tests ---------------------------------

# forward variants of every case: (name, mode, scene kind, flip, outputs)
FWD_VARIANTS = [
    ("composite, per-sample scenes, flip", COMPOSITE, "per", True, "both"),
    ("composite, broadcast scene, adv only", COMPOSITE, "bcast", False, "adv"),
    ("composite, scene_index pool, flip", COMPOSITE, "pool", True, "both"),
    ("warp-only, flip", WARP_ONLY, None, True, "both"),
    ("warp-only, mask_out only", WARP_ONLY, None, False, "mask"),
]
_CACHE = {}


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def fwd_case(cid):
    """The geometry, inputs and float64 results (with their S) of every variant of a forward case."""
    if ("fwd", cid) not in _CACHE:
        _, frame, patch, out, form, misalign, weights, mask_kind, sets = [c for c in FWD_CASES if c[0] == cid][0]
        hw, pad = PATCHES[patch]
        coeffs = coeffs_of(sets)
        N = len(sets)
        P = Paste(coeffs, frame, hw, pad, out, weights)
        d = case_inputs(cid, frame, patch, N, mask_kind, out)
        d.update(P=P, coeffs=coeffs.astype(np.float32), flip=flips_of(N), index=np.array([SCENE_POOL[i % 4] for i in range(N)], np.int32),
                 form=form, misalign=misalign, frame=frame, out=out, sets=sets)
        assert np.array_equal(d["coeffs"].astype(np.float64), coeffs)
        for name, mode, kind, flip, outs in FWD_VARIANTS:
            scene = {"per": d["scenes"], "bcast": d["scenes"][:1], "pool": d["pool"], None: None}[kind]
            kw = dict(mode=mode, flip=d["flip"] if flip else None, scene_index=d["index"] if kind == "pool" else None)
            d[name] = P.forward(scene, d["patch"], d["mask"], **kw) + P.forward(scene, d["patch"], d["mask"], absolute=True, **kw)
        _CACHE[("fwd", cid)] = _freeze(d)
    return _CACHE[("fwd", cid)]


def bwd_case(cid):
    """The geometry, inputs, float64 patch gradient, its S, n_round and the per-texel read counts of a backward case, per mode."""
    if ("bwd", cid) not in _CACHE:
        _, frame, patch, out, weights, mask_kind, names = [c for c in BWD_CASES if c[0] == cid][0]
        hw, pad = PATCHES[patch]
        coeffs = coeffs_of(names)
        N = len(names)
        P = Paste(coeffs, frame, hw, pad, out, weights)
        d = case_inputs(cid, frame, patch, N, mask_kind, out)
        d.update(P=P, coeffs=coeffs.astype(np.float32), flip=flips_of(N), frame=frame, out=out, names=names)
        assert np.array_equal(d["coeffs"].astype(np.float64), coeffs)
        for mode in (COMPOSITE, WARP_ONLY):
            d[mode] = {"g": P.backward(d["g_adv"], d["mask"], mode, d["flip"]),
                       "S": P.backward(d["g_adv"], d["mask"], mode, d["flip"], absolute=True),
                       "n_round": n_bwd(P, mode, d["mask"]),
                       "unread": (P.reads(d["mask"] if mode == COMPOSITE else None).sum(0) == 0).reshape(hw)}
        _CACHE[("bwd", cid)] = _freeze(d)
    return _CACHE[("bwd", cid)]
