"""K24 (tube-light compose and commit) in the ISA hipcc emits -- no GPU needed, hipcc cross-compiles.

A compile is not a run: this pins only what the text of the code object can show.

  * no kernel uses scratch memory or spills a register;
  * the wide compose kernel stores the patch with 16-byte stores;
  * the compose kernels' double arithmetic is not contracted: the distance |k x - y + b| keeps its product and its two sums
    (``#pragma clang fp contract(off)``), and every fused multiply-add in the kernel belongs to the expansion of an IEEE
    division -- counted against a probe kernel holding exactly one division, compiled here with the same flags;
  * the fp32 tail likewise: one v_add_f32 per texel, fused operations only inside the ``/ 255`` divisions.
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "depthmodelhardening_amd", "csrc")
NAMES = ("tube_light_compose_kernel", "tube_light_compose_scalar_kernel", "tube_light_commit_kernel")
PROBE = """#include <hip/hip_runtime.h>
__global__ void probe64(const double* a, double* o) { o[threadIdx.x] = a[threadIdx.x] / a[threadIdx.x + 64]; }
__global__ void probe32(const float* a, float* o) { o[threadIdx.x] = a[threadIdx.x] / a[threadIdx.x + 64]; }
"""


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    return None


def _bodies(isa):
    return {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\S+):.*?\n(.*?)\.Lfunc_end\d+:", isa, re.S | re.M)}


def _count(body, pattern):
    return len(re.findall(r"^\s*(?:%s)\b" % pattern, body, re.M))


FUSED64 = r"v_(?:fma|fmac)_f64\w*"
FUSED32 = r"v_(?:pk_)?(?:fma|fmac|mad|mac)_\w*f32\w*"


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """({short name: (metadata text, body text)} of tube_light.hip's kernels, fused operations per fp64 division, per fp32
    division), all compiled with build.py's flags."""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    from depthmodelhardening_amd.build import FLAGS
    tmp = str(tmp_path_factory.mktemp("isa"))
    flags = [f for f in FLAGS if f != "-fPIC"]
    probe = os.path.join(tmp, "probe.hip")
    with open(probe, "w") as f:
        f.write(PROBE)
    texts = []
    for src in (os.path.join(CSRC, "tube_light.hip"), probe):
        out = os.path.join(tmp, os.path.basename(src) + ".s")
        subprocess.run([hipcc] + flags + ["-I" + CSRC, "--offload-device-only", "-S", src, "-o", out], check=True,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        texts.append(open(out).read())
    isa, probe_isa = texts
    found = {}
    for short in NAMES:
        body = [b for n, b in _bodies(isa).items() if re.search(r"\d%sE" % short, n)]
        meta = [m.group(0) for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", isa, re.S)
                if re.search(r"\d%sE" % short, m.group(0))]
        assert len(body) == 1 and len(meta) == 1, (short, len(body), len(meta))
        found[short] = (meta[0], body[0])
    pb = _bodies(probe_isa)
    (p64,) = [b for n, b in pb.items() if "probe64" in n]
    (p32,) = [b for n, b in pb.items() if "probe32" in n]
    assert _count(p64, r"v_div_fixup_f64") == 1 and _count(p32, r"v_div_fixup_f32") == 1
    return found, _count(p64, FUSED64), _count(p32, FUSED32)


def _field(meta, name):
    return int(re.search(r"\.%s:\s+(\d+)" % name, meta).group(1))


@pytest.mark.parametrize("name", NAMES)
def test_no_scratch_no_spills(compiled, name):
    meta, body = compiled[0][name]
    assert _field(meta, "private_segment_fixed_size") == 0, meta
    assert _field(meta, "vgpr_spill_count") == 0 and _field(meta, "sgpr_spill_count") == 0, meta
    assert "scratch_" not in body


def test_patch_stores_are_wide(compiled):
    _, body = compiled[0]["tube_light_compose_kernel"]
    assert _count(body, r"global_store_dwordx4") == 3            # one per channel: four texels each
    assert _count(body, r"global_store_dword(?:x2|x3)?") == 0


@pytest.mark.parametrize("name,pixels", [("tube_light_compose_kernel", 4), ("tube_light_compose_scalar_kernel", 1)])
def test_compose_is_not_contracted(compiled, name, pixels):
    found, per_div64, per_div32 = compiled
    _, body = found[name]
    div64, div32 = _count(body, r"v_div_fixup_f64"), _count(body, r"v_div_fixup_f32")
    assert div64 == 2 * pixels and div32 == 3 * pixels, (div64, div32)      # / s and beta / (d d); / 255 per channel
    # every fused fp64 operation is a division's: none is left over for k x - y + b, d d, (c att) 255
    assert _count(body, FUSED64) == per_div64 * div64, (_count(body, FUSED64), per_div64, div64)
    assert _count(body, r"v_add_f64") == 2 * pixels                        # k x - y, ... + b
    assert _count(body, r"v_mul_f64") >= 8 * pixels                                       # k x, d d, c att (3), ... 255 (3) per pixel
    assert _count(body, FUSED32) == per_div32 * div32, (_count(body, FUSED32), per_div32, div32)
    assert _count(body, r"v_add_f32\w*") == 3 * pixels                     # fp32 base + fp32 light, one per texel
    assert _count(body, r"v_cvt_f32_f64\w*") == 3 * pixels                 # the one rounding to fp32 per texel
