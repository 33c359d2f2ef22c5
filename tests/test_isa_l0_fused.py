"""K23 (the fused L0 update) in the ISA hipcc emits -- no GPU needed, hipcc cross-compiles.

A compile is not a run: this pins only what the text of the code object can show.

  * neither form of the kernel uses scratch memory or spills a register;
  * the 4-pixel form streams the patch with 16-byte global loads and stores;
  * the division is the correctly rounded expansion (v_div_scale / v_div_fmas / v_div_fixup), not a bare v_rcp_f32 product.  That
    expansion and the square root's correction hold v_fma_f32 of their own, so fused multiply-adds cannot be forbidden wholesale
    here as tests/test_isa_apgd.py does: that the update's own products and sums are rounded one by one is shown on the GPU,
    bit for bit against the numpy restatement (tests/test_gpu_l0_fused.py);
  * no scalar-memory write of any kind in the body.
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "depthmodelhardening_amd", "csrc")
FORMS = {"vector": "l0_fused_kernelILi4E", "scalar": "l0_fused_kernelILi1E"}
SCALAR_WRITES = ("s_" + "store", "s_buffer_" + "store", "s_scratch_" + "store", "s_" + "atomic", "s_buffer_" + "atomic",
                 "s_dcache_" + "wb", "s_dcache_" + "discard")


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    return None


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{form: (metadata text, body text)} of l0_fused.hip's two instantiations, compiled with build.py's flags."""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    from depthmodelhardening_amd.build import FLAGS
    out = os.path.join(str(tmp_path_factory.mktemp("isa")), "l0_fused.s")
    flags = [f for f in FLAGS if f != "-fPIC"]
    subprocess.run([hipcc] + flags + ["-I" + CSRC, "--offload-device-only", "-S", os.path.join(CSRC, "l0_fused.hip"), "-o", out],
                   check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    isa = open(out).read()
    found = {}
    for form, short in FORMS.items():
        body = [m.group(2) for m in re.finditer(r"^(_Z\S+):.*?\n(.*?)\.Lfunc_end\d+:", isa, re.S | re.M) if short in m.group(1)]
        meta = [m.group(0) for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", isa, re.S) if short in m.group(0)]
        assert len(body) == 1 and len(meta) == 1, (form, len(body), len(meta))
        found[form] = (meta[0], body[0])
    return found


def _field(meta, name):
    return int(re.search(r"\.%s:\s+(\d+)" % name, meta).group(1))


@pytest.mark.parametrize("form", sorted(FORMS))
def test_no_scratch_no_spills_no_scalar_writes(kernels, form):
    meta, body = kernels[form]
    assert _field(meta, "private_segment_fixed_size") == 0, meta
    assert _field(meta, "vgpr_spill_count") == 0 and _field(meta, "sgpr_spill_count") == 0, meta
    assert "scratch_" not in body
    low = body.lower()
    assert not [w for w in SCALAR_WRITES if w in low]
    assert "v_div_fixup_f32" in body and "v_div_scale_f32" in body and "v_div_fmas_f32" in body
    assert "v_sqrt_f32" in body
    assert "global_atomic_add" in body          # the count and the ticket


def test_vector_form_uses_16_byte_accesses(kernels):
    _, body = kernels["vector"]
    assert len(re.findall(r"global_load_dwordx4", body)) >= 8       # obj, pos, neg, g_adv, m / v of both patterns
    assert len(re.findall(r"global_store_dwordx4", body)) >= 7      # pos, neg, m / v of both patterns, adv
