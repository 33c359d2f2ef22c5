"""The register budget of the persistent Winograd kernels, read from the ISA hipcc emits (no GPU needed: hipcc cross-compiles).

K10 / K17 run one wave per SIMD on all 512 registers; round 6 took the last spilled registers out of every instantiation by reading
the accumulators through asm ``v_accvgpr_read_b32`` and put the Winograd transforms on packed additions.
A change that makes hipcc spill again, or that silently drops the packed forms, shows here before it shows on a GPU.

The same ISA carries two hazards that the compiler's hazard recognizer cannot see, because the instructions involved are asm
statements (the recognizer does not look into them), and that no GPU test can be trusted to catch (a violation corrupts data
now and then, not always):

  * the stream-K partial-item store ``buffer_store_dwordx4 v[a:b]`` needs 2 wait states before the next instruction that writes
    one of its data registers (an asm ``v_pk_mov_b32`` or ``v_accvgpr_read_b32``): otherwise the store may send the NEW values;
  * the asm ``v_accvgpr_read_b32`` of the epilogue may read an MFMA result only 19 wait states after the MFMA's issue: the
    kernels put 20 (``s_nop 7; s_nop 7; s_nop 3``) in front of the first read, which holds only if no MFMA is scheduled
    between those nops and the reads.
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
def isa(tmp_path_factory):
    """{source name: hipcc -S text}, each source compiled once for the whole module."""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    out_dir = str(tmp_path_factory.mktemp("isa"))
    cache = {}

    def get(name):
        if name not in cache:
            out = os.path.join(out_dir, name + ".s")
            subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-I" + os.path.join(REPO, "include"),
                            "-I" + CSRC, "--offload-device-only", "-S", os.path.join(CSRC, name + ".hip"), "-o", out],
                           check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            cache[name] = open(out).read()
        return cache[name]
    return get


def _kernels(isa, stem):
    """{mangled name: (vgpr_spill_count, body text)} of the kernels whose name contains ``stem``."""
    spills = {m.group(1): int(m.group(2)) for m in
              re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", isa) if stem in m.group(1)}
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\S+):.*?\n(.*?)\.Lfunc_end\d+:", isa, re.S | re.M) if stem in m.group(1)}
    return {k: (v, bodies.get(k, "")) for k, v in spills.items()}


@pytest.mark.parametrize("src,stem,count", [("wino_conv", "wino_conv_kernel", 12), ("wino32_conv", "wino32_conv_kernel", 2)])
def test_no_spilled_registers_and_packed_transforms(isa, src, stem, count):
    ks = _kernels(isa(src), stem)
    assert len(ks) == count, sorted(ks)
    for name, (spilled, body) in ks.items():
        assert spilled == 0, (name, spilled)
        assert "scratch_" not in body, name
        assert body.count("v_pk_add_f32") >= 100, (name, body.count("v_pk_add_f32"))    # both transforms + the epilogue
        reads = body.count("v_accvgpr_read_b32")
        assert 256 <= reads <= 2 * 256 + 64, (name, reads)      # every accumulator once per epilogue copy (whole / partial item)


# ---- hazard checks -------------------------------------------------------------------------------------------------------------

_LABEL = re.compile(r"^[.\w$]+:")
_VREG = re.compile(r"^v(\d+)$|^v\[(\d+):(\d+)\]$")
# instructions without a vector destination register: vector-memory writes and LDS writes (their first operand is an address or
# the data); scalar instructions never write a VGPR
_NO_VDST = re.compile(r"^(buffer|global|flat)_store_|^ds_write")
# control transfers: the instruction that follows in the text is not necessarily the next one executed
_BRANCH = re.compile(r"^s_(branch|cbranch_\w+|setpc_b64|endpgm\w*)$")


def _instructions(body):
    """[(mnemonic, [operands], line number)] of an ISA text: comments, directives and empty lines dropped, labels kept as
    ("<label>", [], n) (a fall-through point, not an instruction)."""
    out = []
    for n, line in enumerate(body.splitlines()):
        code = line.split(";", 1)[0].strip()
        if not code:
            continue
        if _LABEL.match(code):
            out.append(("<label>", [], n))
            continue
        if code.startswith("."):
            continue
        parts = code.split(None, 1)
        ops = [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []
        out.append((parts[0], ops, n))
    return out


def _vregs(operand):
    m = _VREG.match(operand)
    if not m:
        return set()
    if m.group(1) is not None:
        return {int(m.group(1))}
    return set(range(int(m.group(2)), int(m.group(3)) + 1))


def _written_vregs(mnemonic, ops):
    """The VGPRs an instruction writes: the first operand of every vector (VALU, MFMA, load, returning atomic) instruction."""
    if mnemonic.startswith("s_") or mnemonic == "<label>" or _NO_VDST.match(mnemonic) or not ops:
        return set()
    regs = _vregs(ops[0])
    if mnemonic.startswith("v_swap"):
        regs |= _vregs(ops[1])
    return regs


def _wait_states(mnemonic, ops):
    if mnemonic == "<label>":
        return 0
    if mnemonic == "s_nop":
        return int(ops[0], 0) + 1
    return 1


def store_data_hazards(ins, need=2):
    """Every ``buffer_store_dwordx4 v[a:b]`` must be followed by ``need`` wait states (``s_nop N`` = N + 1, any other instruction
    = 1) before the next instruction that writes one of v[a..b].  Labels are passed through (fall-through); a control transfer
    reached before the wait states are complete is reported too (its target is not checked).  Returns [(line, reason)]."""
    found = []
    for i, (mn, ops, line) in enumerate(ins):
        if mn != "buffer_store_dwordx4":
            continue
        data = _vregs(ops[0])
        assert len(data) == 4, (line, ops)
        waited = 0
        for mn2, ops2, line2 in ins[i + 1:]:
            if waited >= need:
                break
            if _written_vregs(mn2, ops2) & data:
                found.append((line, "v%d..v%d rewritten by %s at line %d after %d wait state(s)" % (
                    min(data), max(data), mn2, line2, waited)))
                break
            if _BRANCH.match(mn2):
                found.append((line, "%s at line %d after %d wait state(s)" % (mn2, line2, waited)))
                break
            waited += _wait_states(mn2, ops2)
        else:
            if waited < need:
                found.append((line, "kernel ends after %d wait state(s)" % waited))
    return found


def _epilogues(ins):
    """Indices of the 20-wait-state blocks (s_nop 7; s_nop 7; s_nop 3) that open an epilogue's accumulator reads."""
    seq = [(mn, tuple(ops)) for mn, ops, _ in ins]
    return [i for i in range(len(seq) - 2)
            if seq[i] == ("s_nop", ("7",)) and seq[i + 1] == ("s_nop", ("7",)) and seq[i + 2] == ("s_nop", ("3",))]


def accumulator_read_hazards(ins):
    """From each 20-wait-state block to the next one (or the end of the kernel): no ``v_mfma`` before the first
    ``v_accvgpr_read_b32``, and none between the first and the last read of that epilogue.  Returns [(line, reason)]."""
    found = []
    starts = _epilogues(ins)
    if not starts:
        return [(0, "no 20-wait-state block (s_nop 7; s_nop 7; s_nop 3) found")]
    for s, e in zip(starts, starts[1:] + [len(ins)]):
        reads = [i for i in range(s + 3, e) if ins[i][0] == "v_accvgpr_read_b32"]
        if not reads:
            found.append((ins[s][2], "no v_accvgpr_read_b32 after the wait states"))
            continue
        for i in range(s + 3, reads[-1]):
            if ins[i][0].startswith("v_mfma"):
                where = "before the first" if i < reads[0] else "between two"
                found.append((ins[i][2], "%s %s v_accvgpr_read_b32 of the epilogue at line %d" % (ins[i][0], where, ins[s][2])))
    return found


def _sk_kernels(isa_text, stem, sk_suffix):
    return {n: body for n, (_, body) in _kernels(isa_text, stem).items() if n.endswith(sk_suffix)}


# stream-K instantiations: wino_conv_kernel<TRW, FLAT, EPI, SK = true> (six) and wino32_conv_kernel<SK = true>
@pytest.mark.parametrize("src,stem,sk_suffix,count", [("wino_conv", "wino_conv_kernel", "ELb1EEEvNS_5WArgsE", 6),
                                                      ("wino32_conv", "wino32_conv_kernel", "ILb1EEEvNS_7W32ArgsE", 1)])
def test_stream_k_partial_store_data_hazard(isa, src, stem, sk_suffix, count):
    ks = _sk_kernels(isa(src), stem, sk_suffix)
    assert len(ks) == count, sorted(ks)
    for name, body in sorted(ks.items()):
        ins = _instructions(body)
        stores = sum(1 for mn, _, _ in ins if mn == "buffer_store_dwordx4")
        assert stores >= 16, (name, stores)         # the partial-item path: one 16-byte store per output channel of a lane
        bad = store_data_hazards(ins)
        print("%s: %d partial-item stores, %d hazards" % (name, stores, len(bad)))
        assert not bad, (name, bad[:8])


@pytest.mark.parametrize("src,stem,sk_suffix,count", [("wino_conv", "wino_conv_kernel", "ELb1EEEvNS_5WArgsE", 6),
                                                      ("wino32_conv", "wino32_conv_kernel", "ILb1EEEvNS_7W32ArgsE", 1)])
def test_no_mfma_between_the_wait_states_and_the_accumulator_reads(isa, src, stem, sk_suffix, count):
    ks = _sk_kernels(isa(src), stem, sk_suffix)
    assert len(ks) == count, sorted(ks)
    for name, body in sorted(ks.items()):
        ins = _instructions(body)
        assert _epilogues(ins), name
        bad = accumulator_read_hazards(ins)
        assert not bad, (name, bad[:8])


_GOOD = """
    buffer_store_dwordx4 v[22:25], v81, s[40:43], s4 offen
    ;;#ASMSTART
    s_nop 1
    ;;#ASMEND
.LBB3_264:
    v_pk_mov_b32 v[22:23], v[30:31], v[32:33] op_sel:[0,0]
    s_nop 7
    s_nop 7
    s_nop 3
    v_accvgpr_read_b32 v40, a0
    v_accvgpr_read_b32 v41, a1
    v_mfma_f32_32x32x2_f32 a[0:15], v1, v2, a[0:15]
"""


def test_hazard_checker_reports_what_it_is_built_to_find():
    """The checker can fail: the nop taken out of a store's shadow, a branch in its place, an MFMA moved between the wait states
    and the reads, or between two reads -- each is reported; the intact snippet is not."""
    ok = _instructions(_GOOD)
    assert store_data_hazards(ok) == [] and accumulator_read_hazards(ok) == []
    no_nop = _instructions(_GOOD.replace("s_nop 1\n", ""))
    bad = store_data_hazards(no_nop)
    assert len(bad) == 1 and "v_pk_mov_b32" in bad[0][1], bad
    short = _instructions(_GOOD.replace("s_nop 1\n", "s_nop 0\n"))       # one wait state: still one short
    assert len(store_data_hazards(short)) == 1
    other_reg = _instructions(_GOOD.replace("s_nop 1\n", "").replace("v_pk_mov_b32 v[22:23]", "v_pk_mov_b32 v[26:27]"))
    assert store_data_hazards(other_reg) == []           # a write of OTHER registers is no hazard, and 2 instructions follow
    branch = _instructions(_GOOD.replace("s_nop 1\n", "s_cbranch_vccz .LBB3_264\n"))
    assert len(store_data_hazards(branch)) == 1
    mfma_first = _instructions(_GOOD.replace("    s_nop 3\n", "    s_nop 3\n    v_mfma_f32_32x32x2_f32 a[0:15], v1, v2, a[0:15]\n"))
    bad = accumulator_read_hazards(mfma_first)
    assert len(bad) == 1 and "before the first" in bad[0][1], bad
    mfma_between = _instructions(_GOOD.replace("v_accvgpr_read_b32 v41, a1\n",
                                               "v_mfma_f32_32x32x2_f32 a[0:15], v1, v2, a[0:15]\n    v_accvgpr_read_b32 v41, a1\n"))
    bad = accumulator_read_hazards(mfma_between)
    assert len(bad) == 1 and "between two" in bad[0][1], bad
    assert accumulator_read_hazards(_instructions(_GOOD.replace("    s_nop 3\n", ""))) != []     # 16 wait states: not the block
