"""The sampler's GEMM launches end without a load (csrc/gemm.h: epi_prefetch).

A reverse-sampling step is a chain of three dependent launches, so whatever a work-group does behind its last MFMA is latency of the
step.  What the epilogues of these launches read from global memory - the bias, the hidden layers' PReLU slope, and for the out layer
(EPI_TANH_REV) the work-group's own tile of the sampler state - is known before the K loop, so it is requested there and waits in
registers.  Left in the epilogue the state was four load / wait / update / store round trips in a row per work-group.

This cross-compiles the kernels for gfx950 (no GPU needed) and checks the generated code of the instantiations the host's size rule
dispatches for the sampler: fused reverse updates run on launches of at most FUSE_REV_MAX_ROWS rows, which is the row count up to which
NT launches take the 32x32 tile on the 16-wide MFMA (Cfg4, nt32_max_rows), and k_sample_persist runs on that tile.  The tiles on the
32-wide MFMA (a forced tile, SDRM_FUSE_REV=2) keep the state load in their epilogue: 16 registers per accumulator tile do not fit their
register budgets.

  * gemm_kernel<Cfg4, .., EPI_TANH_REV> and gemm_kernel<Cfg4, .., EPI_BIAS_PRELU>: no global, buffer or flat load behind the last
    v_mfma, no scratch;
  * k_sample_persist<Cfg4>: the last v_mfma of the step loop's body is the out layer's; between it and the sign-in of the hand-shake
    that follows the layer (a global atomic) there is no such load, and the kernel has no scratch.
"""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "sdrm_amd", "csrc")

VMEM_LOAD = re.compile(r"^(global|buffer|flat|scratch)_load")


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    pytest.skip("hipcc not available")


def _host_source():
    return open(os.path.join(CSRC, "sdrm_hip.hip")).read()


def _tile_cfg4():
    m = re.search(r"typedef\s+(TileCfg<[^>]*>)\s+Cfg4\s*;", _host_source())
    assert m, "typedef TileCfg<...> Cfg4 not found in csrc/sdrm_hip.hip"
    return "sdrm::" + m.group(1)


def _kernels(asm):
    """mangled name -> (instructions in program order, scratch bytes)"""
    out, cur, name = {}, None, None
    scratch = {}
    for line in asm.split("\n"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            cur = out.setdefault(name, [])
            continue
        m = re.match(r"^; ScratchSize: (\d+)", line)
        if m and name is not None:
            scratch.setdefault(name, int(m.group(1)))
        if cur is None:
            continue
        t = line.strip()
        if line.startswith("\t") and t and not t.startswith((";", ".")):
            cur.append(t.split(";")[0].strip())
            if t.startswith("s_endpgm"):
                cur = None
    return {k: (v, scratch[k]) for k, v in out.items()}


@pytest.fixture(scope="module")
def sampler_kernels():
    cfg = _tile_cfg4()
    nt = "sdrm::LD_KCONTIG, sdrm::LD_KCONTIG, sdrm::XF_NONE, sdrm::XF_NONE"
    src_text = (f'#include "{CSRC}/sample_persist.h"\n'
                f"template __global__ void sdrm::k_sample_persist<{cfg}>(const sdrm::SamplePersistArgs);\n"
                f"template __global__ void sdrm::gemm_kernel<{cfg}, {nt}, sdrm::EPI_TANH_REV>(const sdrm::GemmArgs);\n"
                f"template __global__ void sdrm::gemm_kernel<{cfg}, {nt}, sdrm::EPI_BIAS_PRELU>(const sdrm::GemmArgs);\n")
    with tempfile.TemporaryDirectory() as d:
        src, out = os.path.join(d, "k.hip"), os.path.join(d, "k.s")
        with open(src, "w") as f:
            f.write(src_text)
        res = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out, src],
                             capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        ks = _kernels(open(out).read())
    (persist,) = [n for n in ks if "k_sample_persist" in n]
    (rev,) = [n for n in ks if "gemm_kernel" in n and n.endswith("ELi6EEEvNS_8GemmArgsE")]
    (hidden,) = [n for n in ks if "gemm_kernel" in n and n.endswith("ELi10EEEvNS_8GemmArgsE")]
    return {"persist": ks[persist], "rev": ks[rev], "hidden": ks[hidden]}


def test_fused_reverse_update_runs_on_the_prefetching_tile():
    """What the other tests lean on: the size rule sends every fused launch to Cfg4, a tile on the 16-wide MFMA."""
    src = _host_source()
    fuse = re.search(r"constexpr int FUSE_REV_MAX_ROWS = (\d+);", src)
    nt32 = re.search(r"int nt32_max_rows = (\d+);", src)
    assert fuse and nt32
    assert int(fuse.group(1)) <= int(nt32.group(1)), "fused launches above the 32x32 tile's row limit would run on a tile that does not prefetch"
    assert re.search(r"return M <= nt32_rows \? 4 : 0;", src), "choose_cfg no longer picks Cfg4 below the row limit"
    assert re.search(r"k_sample_persist<Cfg4>", src)
    args = [a.strip() for a in re.match(r"sdrm::TileCfg<(.*)>", _tile_cfg4()).group(1).split(",")]
    assert len(args) >= 7 and int(args[6]) == 16, args   # MF: the prefetch is compiled for the 16-wide MFMA


@pytest.mark.parametrize("kind", ["rev", "hidden"])
def test_no_load_behind_the_last_mfma(sampler_kernels, kind):
    ins, scratch = sampler_kernels[kind]
    assert scratch == 0, scratch
    mf = [i for i, x in enumerate(ins) if x.startswith("v_mfma")]
    assert mf
    late = [x for x in ins[mf[-1]:] if VMEM_LOAD.match(x)]
    assert not late, late
    stores = [x for x in ins[mf[-1]:] if x.startswith("global_store_dword")]
    assert len(stores) >= 4, stores   # the epilogue IS behind the last MFMA (this lane's four accumulator rows; X and U for the out layer)
    # and the loads sit in front of the loop, among the operand loads of the prologue (buffer_load_dwordx4): the bias and the slope
    # (global_load_dword), the lane's four state elements (buffer_load_dword)
    early = [x for x in ins[:mf[0]] if VMEM_LOAD.match(x)]
    assert sum(1 for x in early if x.startswith("global_load_dword ")) >= (1 if kind == "rev" else 2), early
    assert sum(1 for x in early if x.startswith("buffer_load_dword ")) == (4 if kind == "rev" else 0), early


def test_persistent_sampler_out_layer_loads_nothing_behind_its_mfmas(sampler_kernels):
    ins, scratch = sampler_kernels["persist"]
    assert scratch == 0, scratch
    mf = [i for i, x in enumerate(ins) if x.startswith("v_mfma")]
    assert mf
    tail = ins[mf[-1]:]
    sign = next((i for i, x in enumerate(tail) if x.startswith("global_atomic")), None)
    assert sign is not None, "the hand-shake behind the out layer was not found"
    region = tail[:sign]
    # the out layer's epilogue: the reverse update (its IEEE division) and the stores of X and U
    assert sum(1 for x in region if x.startswith("v_div_fixup_f32")) >= 4
    assert sum(1 for x in region if x.startswith("global_store_dword")) >= 8
    late = [x for x in region if VMEM_LOAD.match(x)]
    assert not late, late
    # the state elements were written by the previous step of this launch: their loads are served by the L2 like the A operand's
    state = [x for x in ins if x.startswith("buffer_load_dword ")]
    assert len(state) == 4 and all(re.search(r"\bsc1\b", x) for x in state), state
