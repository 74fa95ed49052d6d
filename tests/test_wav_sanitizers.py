"""CPU: the RIFF/WAVE header parser and writer (svt_wav_parse, svt_wav_header; svt_speechbrain_amd/csrc/host.cpp) built with
AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone program (`make -C svt_speechbrain_amd/csrc san_wav`,
tests/cabi/wav_san_driver.cpp) and run as a child process: every fixture file of tests/test_wav_host.py, whole, as a prefix and as a file cut
at every length in heap buffers of exactly that size, and 20 000 seeded one- and two-byte mutations of their headers.  The driver asserts
only that nothing is read out of bounds, the return code is a documented one and `out` stays untouched unless a header was accepted; what
each file parses TO is tests/test_wav_host.py's business."""
import os
import re
import subprocess

import pytest

import wav_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svt_speechbrain_amd", "csrc")
BIN = os.path.join(CSRC, "build_san", "wav_san_test")
MUTATIONS = 20000


@pytest.fixture(scope="module")
def san_bin():
    r = subprocess.run(["make", "-C", CSRC, "san_wav"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return BIN


def test_parser_and_header_writer_under_sanitizers(san_bin, tmp_path):
    paths = []
    for name, data in sorted({**{k: v[0] for k, v in WC.well_formed().items()}, **WC.refused()}.items()):
        p = tmp_path / f"{name}.wav"
        p.write_bytes(data)
        paths.append(str(p))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([san_bin, "20261020", str(MUTATIONS), *paths], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout}\n{r.stderr}"
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    m = re.fullmatch(r"wav ok: (\d+) calls, (\d+) parsed, (\d+) asked for more, (\d+) refused\n", r.stdout)
    assert m, r.stdout
    calls, ok, more, refused = map(int, m.groups())
    assert calls == ok + more + refused and calls > 2 * MUTATIONS
    assert ok > 1000 and more > 1000 and refused > 1000     # the mutations reach all three outcomes
