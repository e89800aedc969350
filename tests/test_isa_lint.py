"""ISA lint of the row-owned kernels (csrc/rowchain.h, csrc/dgrad_rows.h): their MFMAs are inline asm with the accumulator tied
in place (the register allocator otherwise renames accumulators inside the K loops and copies them back by the hundred), so the
compiler's hazard recogniser does not see them.  The sources guard the two places where compiler-made VALU code meets the
accumulators (rc_acc_begin / rc_acc_settle); this test cross-compiles the kernels for gfx950 (no GPU needed) and checks the
generated code for any other:

  * no accumulator copy or write (v_accvgpr_*) inside a K loop, no scratch access inside a K loop;
  * an accumulator write by VALU (v_accvgpr_write / v_accvgpr_mov) is never closer than two wait states to the next MFMA;
  * the first accumulator read (v_accvgpr_read) after an MFMA is separated from it by at least 18 wait states of s_nop
    (v_mfma_f32_16x16x4_f32: 8 passes; the CDNA3 ISA guide asks for 11 before a VALU read of the result);
  * no VALU instruction inside the K loops of the dgrad kernels at all (operands by raw buffer loads with scalar offsets).

Every instantiation the host can launch is compiled (16 row-owned cases, 8 strip widths: about five minutes on one core), and
test_every_launched_instantiation_is_linted holds the lists below to the kernels csrc/sdrm_hip.hip really instantiates: it
cross-compiles that translation unit for the device and compares the symbols.
"""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "sdrm_amd", "csrc")


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    pytest.skip("hipcc not available")


def _device_asm(src: str, *defines: str) -> str:
    """gfx950 assembly of the device side of the HIP source file `src`."""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        res = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", *defines, "-o", out, src],
                             capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        return open(out).read()


def _compile(instantiations: str, header: str = "rows48.h") -> str:
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "k.hip")
        with open(src, "w") as f:
            f.write(f'#include "{CSRC}/{header}"\n' + instantiations)
        return _device_asm(src)


def _kernels(asm: str):
    """name -> list of instruction strings (labels kept as 'LABEL name')."""
    out, cur = {}, None
    for line in asm.split("\n"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        t = line.strip()
        if re.match(r"^\.LBB\d+_\d+:", t):
            cur.append("LABEL " + t.split(":")[0])
        elif line.startswith("\t") and t and not t.startswith(";") and not t.startswith("."):
            cur.append(t.split(";")[0].strip())
            if t.startswith("s_endpgm"):
                cur = None
    return out


def _loops(ins):
    """(start, end) index ranges of the basic-block loops: a label and the first backward branch to it."""
    labels = {x.split()[1]: i for i, x in enumerate(ins) if x.startswith("LABEL ")}
    loops = []
    for i, x in enumerate(ins):
        m = re.match(r"s_cbranch_\w+ (\.LBB\d+_\d+)", x)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            loops.append((labels[m.group(1)], i))
    return loops


def _wait_states(x):
    m = re.match(r"s_nop (\d+)", x)
    return int(m.group(1)) + 1 if m else (0 if x.startswith("LABEL") else 1)


VALU_OK_IN_LOOP = ("v_mfma",)


# Every instantiation the host can launch (csrc/sdrm_hip.hip; test_every_launched_instantiation_is_linted holds these lists to it): the
# column tiles CT = padded width / 32, both forms of the last K-step (the host takes the compact one by rc_light_klast(W, WP), which every
# CT can meet), 1 / 2 / 4 work-groups per row group of the 48-row kernels, and the strip widths NT of k_wgrad_strips.
LINT_CT = [4, 5, 6, 7, 8, 9, 10, 11]
LINT_LIGHT = [False, True]
LINT_PARTS = [1, 2, 4]
LINT_NT = [4, 5, 6, 7, 8, 9, 10, 11]

# the asm-MFMA kernel templates and the argument struct each takes
ROW_OWNED = {"k_dgrad_chain": "DgradChainArgs", "k_dgrad_rows": "DgradRowsArgs", "k_row_fwd": "RowChainArgs",
             "k_rows48_fwd": "RowChainArgs", "k_rows48_dgrad_chain": "DgradChain48Args"}


def _row_owned_instantiations(ct, lightb):
    """(kernel, template arguments) of everything test_row_owned_kernels_isa compiles for one (CT, LIGHT): the 96-row kernels; the same
    step on 48-row work-groups (csrc/rows48.h: the same asm MFMAs through the same K-step templates) with one work-group per row group,
    with two (column-split, the form the size rule takes for 1281 .. 2048 users) and with four (batches of at most 1024 users,
    sdrm_debug_set_rows48_split(e, 4)); and, for 4 q + 2 column tiles, their shared-tile form (the waves of a pair split one tile's K-steps),
    which exists for one work-group per group only."""
    inst = [(k, (ct, lightb)) for k in ("k_dgrad_chain", "k_dgrad_rows", "k_row_fwd")]
    for k in ("k_rows48_fwd", "k_rows48_dgrad_chain"):
        inst += [(k, (ct, lightb, parts, False)) for parts in LINT_PARTS]
        if ct % 2:
            inst.append((k, (ct, lightb, 1, True)))
    return inst


def _instantiation(symbol):
    """(kernel, template arguments) of the mangled name of a kernel in namespace sdrm whose template arguments are ints and bools (default
    arguments are part of the name); (kernel, None) for any other."""
    m = re.match(r"_ZN4sdrm(\d+)", symbol)
    if not m:
        return symbol, None
    end = m.end() + int(m.group(1))
    targs = re.match(r"I((?:L[ib]\d+E)+)E", symbol[end:])
    if not targs:
        return symbol[m.end():end], None
    return symbol[m.end():end], tuple(bool(int(v)) if t == "b" else int(v) for t, v in re.findall(r"L([ib])(\d+)E", targs.group(1)))


@pytest.mark.parametrize("lightb", LINT_LIGHT)   # the compact last K-step (340 = 21 * 16 + 4: the headline width), or the plain one
@pytest.mark.parametrize("ct", LINT_CT)
def test_row_owned_kernels_isa(ct, lightb):
    inst = _row_owned_instantiations(ct, lightb)
    asm = _compile("".join("template __global__ void sdrm::%s<%s>(const sdrm::%s);\n" % (k, ", ".join(str(a).lower() for a in targs), ROW_OWNED[k])
                           for k, targs in inst))
    ks = _kernels(asm)
    assert sorted(i for i in map(_instantiation, ks) if i[0] in ROW_OWNED) == sorted(inst)   # (what test_every_launched_instantiation_is_linted reads the library's symbols with)
    names = {"chain": [n for n in ks if "k_dgrad_chain" in n and "rows48" not in n], "rows": [n for n in ks if "k_dgrad_rows" in n],
             "fwd": [n for n in ks if "k_row_fwd" in n], "fwd48": [n for n in ks if "k_rows48_fwd" in n and "ELi2E" not in n and "ELi4E" not in n and "ELi1ELb1E" not in n],
             "chain48": [n for n in ks if "k_rows48_dgrad_chain" in n and "ELi2E" not in n and "ELi4E" not in n and "ELi1ELb1E" not in n],
             "fwd48x2": [n for n in ks if "k_rows48_fwd" in n and "ELi2E" in n],
             "chain48x2": [n for n in ks if "k_rows48_dgrad_chain" in n and "ELi2E" in n],
             "fwd48x4": [n for n in ks if "k_rows48_fwd" in n and "ELi4E" in n],
             "chain48x4": [n for n in ks if "k_rows48_dgrad_chain" in n and "ELi4E" in n]}
    if ct % 2:
        names["fwd48s"] = [n for n in ks if "k_rows48_fwd" in n and "ELi1ELb1E" in n]
        names["chain48s"] = [n for n in ks if "k_rows48_dgrad_chain" in n and "ELi1ELb1E" in n]
    assert all(len(v) == 1 for v in names.values()), names
    for kind, (name,) in names.items():
        ins = ks[name]
        mf = [i for i, x in enumerate(ins) if x.startswith("v_mfma")]
        assert len(mf) >= (100 if "48" not in kind else 12), (kind, len(mf))
        # K loops: the loops that hold MFMAs
        loops = _loops(ins)
        inner = [(a, b) for a, b in loops if not any((c, d) != (a, b) and a <= c and d <= b for c, d in loops)]
        # (the layer loops have barriers, a K loop has none)
        kloops = [(a, b) for a, b in inner if sum(1 for x in ins[a:b] if x.startswith("v_mfma")) >= 24 and "s_barrier" not in ins[a:b]]
        # (a K loop of a single trip is straight-line code: the narrowest nets of the dgrad kernels)
        assert kloops or (not kind.startswith("fwd") and ct <= 7), kind   # (up to 14 K-steps the dgrads' main loop is a single trip of four)
        for a, b in kloops:
            body = ins[a:b]
            assert not [x for x in body if x.startswith("v_accvgpr")], (kind, "accumulator copies inside a K loop")
            assert not [x for x in body if x.startswith("scratch_")], (kind, "scratch access inside a K loop")
            if not kind.startswith("fwd"):
                valu = [x for x in body if x.startswith("v_") and not x.startswith(VALU_OK_IN_LOOP)]
                assert not valu, (kind, "VALU inside a K loop", valu[:4])
            else:
                # the forward keeps a handful per pair of K-steps: LDS addresses of the A fragment reads and of the stream chunks
                valu = [x for x in body if x.startswith("v_") and not x.startswith(VALU_OK_IN_LOOP)]
                assert len(valu) <= 16, (kind, len(valu), valu[:6])
        # hazards around the asm MFMAs
        for i in mf:
            ws = 0
            for j in range(i - 1, max(i - 4, -1), -1):
                x = ins[j]
                if x.startswith(("v_accvgpr_write", "v_accvgpr_mov")):
                    assert ws >= 2, (kind, "VALU write of an accumulator %d wait states before an MFMA" % ws, ins[j:i + 1])
                ws += _wait_states(x)
                if ws >= 2:
                    break
        # accumulator reads: along every path out of an MFMA (branches followed), 18 wait states of s_nop come first
        labels = {x.split()[1]: i for i, x in enumerate(ins) if x.startswith("LABEL ")}

        def walk(i, nops, budget, seen):
            while i < len(ins) and budget > 0 and nops < 18:
                x = ins[i]
                if x.startswith("v_mfma") or x.startswith("s_endpgm"):
                    return
                assert not x.startswith("v_accvgpr_read"), (kind, "accumulator read %d nop states after an MFMA" % nops, ins[max(0, i - 6):i + 1])
                m = re.match(r"s_(c?branch)\w* (\.LBB\d+_\d+)", x)
                if m:
                    tgt = labels[m.group(2)]
                    if (tgt, nops) not in seen:
                        seen.add((tgt, nops))
                        walk(tgt, nops, budget - 1, seen)
                    if m.group(1) == "branch":
                        return
                nops += _wait_states(x) if x.startswith("s_nop") else 0
                i += 1
                budget -= 1

        for i in mf:
            if not ins[i + 1].startswith("v_mfma"):
                walk(i + 1, 0, 96, set())


def test_fragment_packing_is_a_bijection():
    """wfrag_index (csrc/elementwise.h) maps the (n, k) of a padded [NP][KP] weight onto the fragment-packed copy the row-owned
    kernels load from - with the compact last K-step (k = 16 klast + j in lane group j, component 0) it must still hit every
    slot exactly once, and rc_light_klast must pick that form exactly when the last padded K-step holds one to four real k.
    Host code, compiled with hipcc and run here."""
    src = r'''
#include <cstdio>
#include <vector>
#include "%s/elementwise.h"
using namespace sdrm;
int main() {
  const int cases[][3] = {{340, 352, 21}, {337, 352, 21}, {180, 192, 11}, {100, 128, -1}, {136, 160, -1}, {352, 352, -1}, {341, 352, -1},
                          {336, 352, -1}, {20, 32, 1}, {16, 32, -1}};
  for (auto& c : cases) {
    const int K = c[0], KP = c[1], want = c[2];
    const int kl = rc_light_klast(K, KP);
    if (kl != want) { printf("rc_light_klast(%%d, %%d) = %%d, expected %%d\n", K, KP, kl, want); return 1; }
    const int NP = KP, NCT = NP / 16;
    std::vector<int> hit((size_t)NP * KP, 0);
    for (int n = 0; n < NP; ++n)
      for (int k = 0; k < KP; ++k) {
        const size_t i = wfrag_index(n, k, NCT, kl);
        if (i >= hit.size()) { printf("index out of range\n"); return 1; }
        ++hit[i];
        // the layout contract of the kernels: tile (k / 16, n / 16) is 256 consecutive floats, lane = 16 * group + n %% 16
        const size_t tile = i / 256, lane = (i %% 256) / 4, comp = i %% 4;
        const int kk = k & 15;
        const bool compact = (k >> 4) == kl;
        const int group = compact ? (kk & 3) : (kk >> 2), e = compact ? (kk >> 2) : (kk & 3);
        if (tile != (size_t)(k >> 4) * NCT + (n >> 4) || lane != (size_t)(16 * group + (n & 15)) || comp != (size_t)e) { printf("layout\n"); return 1; }
      }
    for (int v : hit) if (v != 1) { printf("not a bijection at K = %%d\n", K); return 1; }
  }
  printf("ok\n");
  return 0;
}
''' % CSRC
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "h.hip")
        with open(path, "w") as f:
            f.write(src)
        exe = os.path.join(d, "h")
        res = subprocess.run([_hipcc(), "-O1", "-std=c++17", "--offload-arch=gfx950", "-o", exe, path], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        run = subprocess.run([exe], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr


# NT = 5 alone misses the speed bar 8 * VALU <= MFMA of the strips kernel's K loops, by one address instruction: 16 VALU against 120
# MFMAs as measured (NT 4: 12 / 96, 6: 14 / 144, 7: 16 / 168, 8: 16 / 192, 9: 18 / 216, 10: 20 / 240, 11: 22 / 264).  The bar is about
# speed, not correctness, so that width keeps its measured count as a ceiling of its own; the bar of every other width is unchanged.
STRIPS_VALU_CEILING = {5: 16}


@pytest.mark.parametrize("nt", LINT_NT)
def test_strips_kernel_loop_is_clean(nt):
    """k_wgrad_strips (csrc/wgrad2.h) uses the MFMA builtin: the K loop must hold no accumulator copies (the allocator has been seen
    to rename accumulators inside such loops - 124 v_accvgpr_mov per three K-steps in the 16-wide experiment), no scratch, and only
    a handful of VALU instructions (its staging addresses are buffer resources + scalar offsets).  Every strip width the host launches:
    a K loop of width NT holds 24 NT MFMAs."""
    asm = _compile(f"template __global__ void sdrm::k_wgrad_strips<{nt}>(const sdrm::Wg2Args);\n", "wgrad2.h")
    ks = _kernels(asm)
    (name,) = [n for n in ks if "k_wgrad_strips" in n]
    ins = ks[name]
    assert not [x for x in ins if x.startswith("scratch_")]
    loops = _loops(ins)
    inner = [(a, b) for a, b in loops if not any((c, d) != (a, b) and a <= c and d <= b for c, d in loops)]
    kloops = [(a, b) for a, b in inner if sum(1 for x in ins[a:b] if x.startswith("v_mfma")) >= 24 * nt]
    assert kloops
    for a, b in kloops:
        body = ins[a:b]
        nm = sum(1 for x in body if x.startswith("v_mfma"))
        assert sum(1 for x in body if x.startswith(("v_accvgpr_mov", "v_accvgpr_write"))) == 0
        assert not [x for x in body if x.startswith("scratch_")]
        valu = [x for x in body if x.startswith("v_") and not x.startswith(("v_mfma", "v_accvgpr_read"))]
        if nt in STRIPS_VALU_CEILING:
            assert len(valu) <= STRIPS_VALU_CEILING[nt], (len(valu), nm, valu[:6])
        else:
            assert len(valu) * 8 <= nm, (len(valu), nm, valu[:6])


def test_every_launched_instantiation_is_linted():
    """The lint is what the correctness of the asm-MFMA kernels rests on, so the instantiations the library holds must be the ones it
    compiles, no more and no fewer: csrc/sdrm_hip.hip itself, cross-compiled for the device (about four minutes on one core), and the
    kernels found in it against what the parameter lists above make the lint tests compile.  Equality: a kernel the host can launch and the
    lint never saw fails here, and so does a lint case for a kernel that is gone."""
    library = {}
    for symbol in _kernels(_device_asm(os.path.join(CSRC, "sdrm_hip.hip"), '-DSDRM_SOURCE_HASH="isa-lint"')):
        kernel, targs = _instantiation(symbol)
        library.setdefault(kernel, set()).add(targs)
    linted = {k: set() for k in ROW_OWNED}
    for ct in LINT_CT:
        for lightb in LINT_LIGHT:
            for k, targs in _row_owned_instantiations(ct, lightb):
                linted[k].add(targs)
    linted["k_wgrad_strips"] = {(nt,) for nt in LINT_NT}
    for k, want in linted.items():
        have = library.get(k, set())
        assert have == want, (k, "in the library, not linted:", sorted(have - want), "linted, not in the library:", sorted(want - have))


def _tile_cfg4():
    """The template arguments of the sampler's tile (`typedef TileCfg<...> Cfg4;` in csrc/sdrm_hip.hip, what k_sample_persist is launched with)."""
    m = re.search(r"typedef\s+(TileCfg<[^>]*>)\s+Cfg4\s*;", open(os.path.join(CSRC, "sdrm_hip.hip")).read())
    assert m, "typedef TileCfg<...> Cfg4 not found in csrc/sdrm_hip.hip"
    return "sdrm::" + m.group(1)


def test_persistent_sampler_loads():
    """k_sample_persist (csrc/sample_persist.h) hands activations from work-group to work-group of ONE launch through the XCD's L2: the
    A operand of every layer must be loaded with sc1 (a plain load may be served by a stale line of the CU's L1), the weights need not
    be.  The tile body stages as many A loads as B loads (32 x 32 tiles), so: some loads carry sc1, exactly as many do not, nothing
    spills - and the same body behind a kernel boundary (gemm_kernel, AUX = 0) has none with sc1."""
    cfg = _tile_cfg4()
    asm = _compile(f"template __global__ void sdrm::k_sample_persist<{cfg}>(const sdrm::SamplePersistArgs);\n"
                   f"template __global__ void sdrm::gemm_kernel<{cfg}, sdrm::LD_KCONTIG, sdrm::LD_KCONTIG, sdrm::XF_NONE, sdrm::XF_NONE, "
                   f"sdrm::EPI_TANH_REV>(const sdrm::GemmArgs);\n", "sample_persist.h")
    ks = _kernels(asm)
    (persist,) = [n for n in ks if "k_sample_persist" in n]
    (plain,) = [n for n in ks if "gemm_kernel" in n]

    def loads(name):
        ld = [x for x in ks[name] if x.startswith("buffer_load_dwordx4")]
        return sum(1 for x in ld if re.search(r"\bsc1\b", x)), sum(1 for x in ld if not re.search(r"\bsc1\b", x))
    assert not [x for x in ks[persist] if x.startswith("scratch_")]
    assert sum(1 for x in ks[persist] if x.startswith("v_mfma")) > 0
    coherent, other = loads(persist)
    assert coherent > 0 and coherent == other, (coherent, other)
    coherent0, other0 = loads(plain)
    assert coherent0 == 0 and other0 > 0, (coherent0, other0)


def test_narrow_forward_layer_reads_precede_its_mfmas():
    """k_skinny_fwd4 (csrc/skinny_fwd4.h): a hidden layer of a wave is twelve ds_read_b128 and 48 v_mfma_f32_4x4x1_16b_f32.  Left
    to itself the scheduler pairs every read with its four MFMAs - twelve exposed LDS round trips per layer (1277 cycles measured
    against 711) - so the source pins the reads in front (sched_group_barrier): here the hidden-layer loop must hold no scratch
    access, and at most two LDS reads may follow the first MFMA of the loop body."""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "k.hip")
        with open(src, "w") as f:
            f.write(f'#include "{CSRC}/skinny_fwd4.h"\ntemplate __global__ void sdrm::k_skinny_fwd4<3, 3>(const sdrm::SkStepArgs);\n')
        out = os.path.join(d, "k.s")
        res = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out, src],
                             capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        asm = open(out).read()
    ks = _kernels(asm)
    (name,) = [n for n in ks if "k_skinny_fwd4" in n]
    ins = ks[name]
    assert not [x for x in ins if x.startswith("scratch_")]
    assert sum(1 for x in ins if x.startswith("v_mfma_f32_4x4x1")) == 3 * 48
    loops = _loops(ins)
    hidden = [(a, b) for a, b in loops if sum(1 for x in ins[a:b] if x.startswith("v_mfma_f32_4x4x1")) == 48]
    assert hidden, "the hidden-layer loop was not found"
    for a, b in hidden:
        body = ins[a:b]
        first = next(i for i, x in enumerate(body) if x.startswith("v_mfma_f32_4x4x1"))
        assert sum(1 for x in body[first:] if x.startswith("ds_read_b128")) <= 2, [x for x in body[first:] if x.startswith("ds_read")]
