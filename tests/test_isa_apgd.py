"""K22 (Auto-PGD step and commit) in the ISA hipcc emits -- no GPU needed, hipcc cross-compiles.

A compile is not a run: this pins only what the text of the code object can show.

  * neither kernel uses scratch memory or spills a register;
  * both stream the patch with 16-byte global loads and stores;
  * the step kernel holds no fused multiply-add: its result has to equal the reference's element-wise fp32 expression, where every
    product and sum is rounded on its own (``#pragma clang fp contract(off)`` in apgd1), while hipcc's default contracts.
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "depthmodelhardening_amd", "csrc")


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    return None


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{short name: (metadata text, body text)} of apgd_ops.hip's two kernels, compiled with build.py's flags."""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    from depthmodelhardening_amd.build import FLAGS
    out = os.path.join(str(tmp_path_factory.mktemp("isa")), "apgd_ops.s")
    flags = [f for f in FLAGS if f != "-fPIC"]
    subprocess.run([hipcc] + flags + ["-I" + CSRC, "--offload-device-only", "-S", os.path.join(CSRC, "apgd_ops.hip"), "-o", out],
                   check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    isa = open(out).read()
    found = {}
    for short in ("apgd_step_kernel", "apgd_commit_kernel"):
        body = [m.group(2) for m in re.finditer(r"^(_Z\S+):.*?\n(.*?)\.Lfunc_end\d+:", isa, re.S | re.M) if short in m.group(1)]
        meta = [m.group(0) for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", isa, re.S) if short in m.group(0)]
        assert len(body) == 1 and len(meta) == 1, (short, len(body), len(meta))
        found[short] = (meta[0], body[0])
    return found


def _field(meta, name):
    return int(re.search(r"\.%s:\s+(\d+)" % name, meta).group(1))


@pytest.mark.parametrize("name", ["apgd_step_kernel", "apgd_commit_kernel"])
def test_no_scratch_and_wide_accesses(kernels, name):
    meta, body = kernels[name]
    assert _field(meta, "private_segment_fixed_size") == 0, meta
    assert _field(meta, "vgpr_spill_count") == 0 and _field(meta, "sgpr_spill_count") == 0, meta
    assert "scratch_" not in body
    assert "global_load_dwordx4" in body and "global_store_dwordx4" in body


def test_step_kernel_is_not_contracted(kernels):
    _, body = kernels["apgd_step_kernel"]
    fused = re.findall(r"^\s*(v_(?:pk_)?(?:fma|fmac|mad|mac)_\w*f32\w*)", body, re.M)
    assert not fused, sorted(set(fused))
    assert len(re.findall(r"^\s*v_mul_f32", body, re.M)) >= 3      # ss * sign, (x1 - x) * a, grad2 * (1 - a)
