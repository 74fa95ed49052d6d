"""What hipcc made of the kernels, checked on the built libraries (no GPU needed: llvm-objdump of the gfx950 code objects).

Round 5 found a forward that was not reproducible while other processes used the GPU: hipcc had split a 16-byte load of
`head_dots_kernel` into an OVERLAPPING pair (`global_load_dwordx3 ... offset:4` + `global_load_dwordx2`) and guarded the first use with
its own counted `s_waitcnt vmcnt(N)`; under load the sum of squares of the output norm came out short in ~0.15 % of the forwards
(svt_speechbrain_amd/csrc/stats.hip, tools/determinism_stress.py; three rebuilds without that combination were clean, though a
microbenchmark of the bare pair, tools/microbench/split_load_probe.hip, does not reproduce it).  The kernel now issues loads the compiler
cannot take apart; this test keeps 12-byte vector loads out of every kernel except the one that really reads 7-tap rows (16 + 12 bytes,
not overlapping)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
ALLOWED = ("conv3d_front_f32_kernel",)   # fp32 lip-frame stem: rows of 7 taps = one 16-byte + one 12-byte load at a 16-byte boundary


@pytest.mark.parametrize("lib", ["libsvt_mi355.so", "libsvt_mi355_f16.so"])
def test_no_split_vector_loads(lib):
    src = os.path.join(ROOT, "svt_speechbrain_amd", lib)
    if not os.path.exists(src) or not os.path.exists(OBJDUMP):
        pytest.skip("library or llvm-objdump not present")
    with tempfile.TemporaryDirectory() as d:
        so = os.path.join(d, lib)
        shutil.copy(src, so)
        subprocess.run([OBJDUMP, "--offloading", so], check=True, capture_output=True, cwd=d)   # writes the bundles next to `so`
        objs = [f for f in os.listdir(d) if "amdgcn" in f]
        assert objs, "no gfx950 code object found in " + lib
        bad = []
        n_kernels = 0
        for f in objs:
            dis = subprocess.run([OBJDUMP, "-d", os.path.join(d, f)], check=True, capture_output=True, text=True).stdout
            kernel = None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    kernel = m.group(1)
                    n_kernels += 1
                    continue
                if "load_dwordx3" in line and kernel and not any(a in kernel for a in ALLOWED):
                    bad.append((kernel, line.split("//")[0].strip()))
        assert n_kernels > 100, n_kernels
        assert not bad, bad[:8]


@pytest.mark.parametrize("lib", ["libsvt_mi355.so", "libsvt_mi355_f16.so"])
def test_vmem_table_of_hand_counted_waits(lib):
    """every kernel with hand-written `s_waitcnt vmcnt(N)` is held to the committed table of its VMEM
    instructions and counted waits (tools/isa_vmem_table.py: written when the GPU suite, the soak and the determinism stress were green on
    this code) -- a spill, a split / widened / duplicated load, a wait the compiler added or dropped, or a load moved ACROSS a counted wait
    (the table holds a digest of the VMEM instructions between consecutive counted waits, in program order) changes the table.  Beyond the
    table: no scratch traffic at all in these kernels, and the LDS-DMA GEMM stream issues nothing but 16-byte requests, 16-byte
    bias loads and 8- / 16-byte row stores."""
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_vmem_table as T
    src = os.path.join(ROOT, "svt_speechbrain_amd", lib)
    if not os.path.exists(src) or not os.path.exists(OBJDUMP):
        pytest.skip("library or llvm-objdump not present")
    got = T.table_of(src)
    want = json.load(open(T.TABLE))[lib]
    assert len(got) >= 40, len(got)
    for name, rec in got.items():
        assert not any(m.startswith("scratch_") for m in rec["vmem"]), (name, rec["vmem"])
        if any(f in name for f in T.STREAM_FAMILIES):
            extra = set(rec["vmem"]) - T.STREAM_ALLOWED
            assert not extra, (name, extra)
    assert sorted(got) == sorted(want), (sorted(set(got) ^ set(want))[:6], "kernel set changed: re-validate on the GPU, then python tools/isa_vmem_table.py")
    diff = [(k, got[k], want[k]) for k in got if got[k] != want[k]]
    assert not diff, (diff[:3], "VMEM / wait table changed: re-validate on the GPU, then python tools/isa_vmem_table.py")


def _kernel_names(src):
    """Demangled names of the device kernels of a built library."""
    syms = subprocess.run(["nm", "-C", "--defined-only", src], capture_output=True, text=True).stdout
    if "gemm_pps_kernel" not in syms:   # kernel names live in the device code objects, not in the host symbol table
        import sys
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import isa_vmem_table as T
        syms = "\n".join(subprocess.run(["c++filt"], input="\n".join(
            m for dis in T.disassemble(src) for m in re.findall(r"^[0-9a-f]+ <(\S+)>:", dis, re.M)), capture_output=True, text=True).stdout.splitlines())
    return syms


@pytest.mark.parametrize("lib", ["libsvt_mi355.so", "libsvt_mi355_f16.so"])
def test_shipped_library_holds_only_dispatched_forms(lib):
    """experiment kernels that nothing dispatches (`gemm_p1x_kernel`, the lockstep 8-wave attention, stamped
    diagnostic instantiations) are built by `make DIAG=1` only."""
    src = os.path.join(ROOT, "svt_speechbrain_amd", lib)
    if not os.path.exists(src):
        pytest.skip("library not present")
    syms = _kernel_names(src)
    assert "gemm_pps_kernel" in syms and "flash_attn_stag_kernel" in syms
    for residue in ("gemm_p1x_kernel", "flash_attn_pipe_kernel", "flash_attn_kernel<64, false, 8", "flash_attn_x3_kernel<64, true, 8",
                    "flash_attn_x3_kernel<64, false, 8"):
        assert residue not in syms, residue
    # gemm_pps_kernel<BM, ACT>: the six dispatched instantiations and no other
    got = sorted(set(re.findall(r"gemm_pps_kernel<(\d+), (\d+)>", syms)))
    assert got == sorted((str(bm), str(act)) for bm in (128, 192, 256) for act in (0, 1)), got
    assert len(set(re.findall(r"gemm_pps_kernel<[^>]*>", syms))) == 6
    for m in re.findall(r"gemm_p1w_kernel<([^>]*)>", syms):
        assert m.split(",")[-1].strip() == "false", m   # TR (stamps) only under DIAG


def test_diagnostic_library_holds_no_retired_arms():
    """The A/B arms measured and dropped in rounds 3-5 are gone from the sources, so the diagnostic build (libsvt_mi355_diag.so, made by
    build()) cannot hold them either: the software-pipelined attention, the lockstep non-bias 8-wave attention kernels, the two-slot /
    eight-barrier / stamped / default-store forms of gemm_pps_kernel and the six-slot form of gemm_x3q_kernel.  What stays is
    instrumentation of shipped kernels and the gemm_p1x_kernel candidate."""
    src = os.path.join(ROOT, "svt_speechbrain_amd", "libsvt_mi355_diag.so")
    if not os.path.exists(src):
        pytest.skip("library not present")
    syms = _kernel_names(src)
    assert "gemm_p1x_kernel" in syms and "flash_attn_stag_kernel" in syms and "flash_attn_kernel<64, true, 8>" in syms
    for residue in ("flash_attn_pipe_kernel", "flash_attn_kernel<64, false, 8", "flash_attn_x3_kernel<64, true, 8",
                    "flash_attn_x3_kernel<64, false, 8"):
        assert residue not in syms, residue
    # gemm_pps_kernel<BM, ACT> only (the retired forms were further template arguments)
    pps = set(re.findall(r"gemm_pps_kernel<([^>]*)>", syms))
    assert pps == {f"{bm}, {act}" for bm in (128, 192, 256) for act in (0, 1)}, sorted(pps)
    # gemm_x3q_kernel<F16, BM, OUT, DBG>: the three-slot form only (the six-slot form was a fifth argument)
    x3q = set(re.findall(r"gemm_x3q_kernel<([^>]*)>", syms))
    assert x3q and all(len(m.split(",")) == 4 for m in x3q), sorted(x3q)
