"""What tools/make_goldens_jitter.py and the K33 tests must agree on: the seeded images and drawn transforms of every case, and
Pillow's own chain (torchvision 0.8.2's ColorJitter on PIL images: ImageEnhance.Brightness / Contrast / Color and the HSV hue
step).  tests/golden/pil_jitter.npz holds expected outputs only; the inputs are regenerated from the seeds here.  PIL is imported
inside the functions that need it."""
import hashlib
import itertools
import random

import numpy as np

from depthmodelhardening_amd import color_jitter

OPS = ("brightness", "contrast", "saturation", "hue")
ORDERS = [list(o) for o in itertools.permutations(OPS)]         # all 24
RANGES = ((0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.1, 0.1))      # mono_dataset.py:75-78 through ColorJitter.get_params


def _seed(name):
    return int(hashlib.sha256(name.encode()).hexdigest()[:8], 16)


def image(name, hw, lo=0):
    """uint8 [3, h, w] with values in [lo, 255], seeded by the name."""
    return np.random.RandomState(_seed(name)).randint(lo, 256, size=(3,) + tuple(hw)).astype(np.uint8)


def batch(name, n, hw, lo=0):
    return np.stack([image("%s/%d" % (name, i), hw, lo) for i in range(n)])


def draw(rng, order=None):
    """One ColorJitter.get_params from ``rng``: four uniforms, then the shuffle (or the given order)."""
    f = [rng.uniform(lo, hi) for lo, hi in RANGES]
    if order is None:
        order = list(OPS)
        rng.shuffle(order)
    return color_jitter.JitterParams(*f, list(order))


def order_params(name):
    """24 transforms, one per order, factors drawn from the reference's ranges."""
    rng = random.Random(_seed(name))
    return [draw(rng, o) for o in ORDERS]


def lattice():
    """Every colour with channel values range(0, 256, 3) plus 254 and 255: 88^3 pixels as one image [3, 88, 7744]."""
    v = np.array(list(range(0, 256, 3)) + [254, 255], dtype=np.uint8)
    assert v.size == 88
    return np.ascontiguousarray(np.stack(np.meshgrid(v, v, v, indexing="ij")).reshape(3, 88, 88 * 88))


LATTICE_SHIFTS = (0, 25, 128, 231)
LATTICE_SATURATIONS = (0.8, 1.0, 1.2)


def only(name, factor):
    """A transform of one operation."""
    f = {"brightness": 1.0, "contrast": 1.0, "saturation": 1.0, "hue": 0.0}
    f[name] = factor
    return color_jitter.JitterParams(f["brightness"], f["contrast"], f["saturation"], f["hue"], [name])


def hue_record(shift):
    """The record [1, 8] of one hue step with the byte shift given directly (128 is the shift of no factor in [-0.5, 0.5])."""
    rec = color_jitter.pil_records([only("hue", 0.0)])
    rec[0, 5] = shift
    return rec


TIE = np.broadcast_to(np.array([10, 11], dtype=np.uint8), (3, 1, 2)).copy()      # grey 10 | 11: the mean of L is 10.5, m = 11


def clip_case():
    """Values >= 200 at brightness 1.2 (the 255 clip), then the other three."""
    rng = random.Random(_seed("clip"))
    p = draw(rng, ["brightness", "hue", "contrast", "saturation"])
    p.factors["brightness"] = 1.2
    return image("clip", (9, 12), lo=200), p


def golden_cases():
    """(key, uint8 [B, 3, H, W], B transforms or None).  67 x 259 is more than one workgroup per image and no multiple of a
    workgroup's pixels in either of K33's forms (256 and 1024 pixels per workgroup and round)."""
    cases = [("orders", batch("orders", 24, (13, 21)), order_params("orders"))]
    for hw in ((5, 7), (37, 53), (32, 96), (67, 259)):
        name = "s%dx%d" % hw
        cases.append((name, batch(name, 1, hw), [draw(random.Random(_seed(name)))]))
    rng = random.Random(_seed("mixed"))
    cases.append(("mixed", batch("mixed", 5, (32, 96)), [draw(rng), None, draw(rng), None, draw(rng)]))
    cases.append(("tie", TIE[None], [only("contrast", 0.9)]))
    img, p = clip_case()
    cases.append(("clip", img[None], [p]))
    cases.append(("flat", np.full((1, 3, 4, 6), 77, dtype=np.uint8), [draw(random.Random(_seed("flat")))]))
    cases.append(("hue_zero", batch("hue_zero", 1, (6, 10)), [only("hue", -0.001)]))
    return cases


# ---- Pillow itself
def _to_pil(img):
    from PIL import Image
    return Image.fromarray(np.ascontiguousarray(np.asarray(img).transpose(1, 2, 0)))


def pillow_hue(im, hue_factor, shift=None):
    """torchvision 0.8.2 functional_pil.adjust_hue: ``np_h += np.uint8(hue_factor * 255)`` on the H byte, wrapping."""
    from PIL import Image
    shift = color_jitter.pil_hue_shift(hue_factor) if shift is None else shift
    h, s, v = im.convert("HSV").split()
    np_h = ((np.array(h, dtype=np.uint8).astype(np.int32) + shift) & 255).astype(np.uint8)
    return Image.merge("HSV", (Image.fromarray(np_h), s, v)).convert("RGB")


def pillow_hue_shift(img, shift):
    """uint8 [3, H, W] through the hue step with the byte shift itself."""
    return np.ascontiguousarray(np.array(pillow_hue(_to_pil(img), None, shift)).transpose(2, 0, 1))


def pillow_jitter(img, p):
    """uint8 [3, H, W] through Pillow's chain of ``p`` (None: unchanged)."""
    from PIL import ImageEnhance
    if p is None:
        return np.array(img, copy=True)
    im = _to_pil(img)
    for name in p.order:
        f = p.factors[name]
        if name == "brightness":
            im = ImageEnhance.Brightness(im).enhance(f)
        elif name == "contrast":
            im = ImageEnhance.Contrast(im).enhance(f)
        elif name == "saturation":
            im = ImageEnhance.Color(im).enhance(f)
        else:
            im = pillow_hue(im, f)
    return np.ascontiguousarray(np.array(im).transpose(2, 0, 1))


def pillow_batch(images, params):
    return np.stack([pillow_jitter(img, p) for img, p in zip(images, params)])
