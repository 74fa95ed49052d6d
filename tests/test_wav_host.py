"""CPU: the RIFF/WAVE header parser and writer of the C ABI (svt_wav_parse, svt_wav_header; csrc/host.cpp) through _lib.  Files written
by the stdlib ``wave`` module parse to its own ``getparams()``; hand-built headers cover float, EXTENSIBLE, skipped chunks, open-ended and
overlong data sizes and partial frames; a prefix cut at any length either parses to the same answer or asks for a longer prefix; every
refusal leaves ``out`` as it was; a written header parses back to its arguments and ``wave`` reads our 16-bit files.  Also here: the two
numpy identities the GPU tests' expected values rest on."""
import ctypes
import io
import wave

import numpy as np
import pytest

import wav_cases as WC
from svt_speechbrain_amd import _lib

OK, NEED_MORE, INVALID = 0, 1, -1
FIELDS = [f for f, _ in _lib.WavInfoC._fields_]
PREFILL = dict(format=-7, channels=-6, sample_rate=-5, bits_per_sample=-4, block_align=-3, data_offset=-2, frames=-9)
GOOD = WC.well_formed()
BAD = WC.refused()


def parse(data, head_len=None, file_bytes=None):
    """-> (rc, out as a dict, need_bytes); out is prefilled with PREFILL and the head is an exact-size copy of the prefix."""
    lib = _lib.load()
    head_len = len(data) if head_len is None else head_len
    head = ctypes.create_string_buffer(bytes(data[:head_len]), max(head_len, 1))
    wi = _lib.WavInfoC(**PREFILL)
    need = ctypes.c_int64(-1)
    rc = lib.svt_wav_parse(head, head_len, len(data) if file_bytes is None else file_bytes, ctypes.byref(wi), ctypes.byref(need))
    return rc, {f: getattr(wi, f) for f in FIELDS}, need.value


def test_the_struct_has_the_layout_the_header_declares(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "wi.c"
    src.write_text('#include <stdio.h>\n#include "svt_mi355.h"\nint main(void) {\n  printf("%zu", sizeof(svt_wav_info));\n' +
                   "".join(f'  printf(" %zu", offsetof(svt_wav_info, {f}));\n' for f in FIELDS) +
                   '  printf(" %d %d %d %d", SVT_WAV_NEED_MORE, SVT_PCM_U8, SVT_PCM_F64, SVT_ABI_VERSION);\n  return 0;\n}\n')
    exe = str(tmp_path / "wi")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.WavInfoC)] + [getattr(_lib.WavInfoC, f).offset for f in FIELDS] + [NEED_MORE, 1, 6, 1]


@pytest.mark.parametrize("channels", (1, 2, 3))
@pytest.mark.parametrize("width", (1, 2, 3, 4))
def test_files_of_the_wave_module_parse_to_its_own_parameters(width, channels):
    data = WC.wave_module_file(width, channels)
    with wave.open(io.BytesIO(data), "rb") as w:
        p = w.getparams()
        frames = w.readframes(p.nframes)
    rc, got, _ = parse(data)
    assert rc == OK, _lib.last_error()
    assert (got["channels"], got["bits_per_sample"] // 8, got["sample_rate"], got["frames"]) == (p.nchannels, p.sampwidth, p.framerate, p.nframes)
    assert got["format"] == {1: WC.U8, 2: WC.S16, 3: WC.S24, 4: WC.S32}[width] and got["block_align"] == width * channels
    assert data[got["data_offset"]:got["data_offset"] + got["frames"] * got["block_align"]] == frames


@pytest.mark.parametrize("name", sorted(GOOD))
def test_well_formed_headers(name):
    data, want = GOOD[name]
    rc, got, _ = parse(data)
    assert rc == OK, _lib.last_error()
    assert got == want


@pytest.mark.parametrize("name", sorted(GOOD))
def test_a_prefix_of_any_length_parses_the_same_or_asks_for_more(name):
    data, want = GOOD[name]
    full = want["data_offset"]
    for n in range(0, full + 1):
        rc, got, need = parse(data, head_len=n)
        if rc == OK:
            assert got == want, n
        else:
            assert rc == NEED_MORE, (n, rc, _lib.last_error())
            assert got == PREFILL, n
            assert n < need <= len(data), (n, need)
    assert parse(data, head_len=full)[0] == OK
    # following the requests from an empty prefix arrives, in a few steps, at a prefix that parses
    n, steps = 0, 0
    while True:
        rc, got, need = parse(data, head_len=n)
        if rc == OK:
            break
        n, steps = need, steps + 1
        assert steps < 16
    assert got == want and n <= full


@pytest.mark.parametrize("name", sorted(BAD))
def test_refusals_leave_out_untouched(name):
    data = BAD[name]
    rc, got, _ = parse(data)
    assert rc == INVALID, name
    assert got == PREFILL
    assert _lib.last_error().startswith("svt_wav_parse"), _lib.last_error()


@pytest.mark.parametrize("name", sorted(GOOD))
def test_a_file_cut_before_its_data_chunk_is_refused(name):
    """Every truncation: the FILE (not just the prefix) ends at n, for every n short of the data chunk's header."""
    data, want = GOOD[name]
    for n in range(0, want["data_offset"]):
        rc, got, _ = parse(data[:n])
        assert rc == INVALID and got == PREFILL, (n, rc)
        assert _lib.last_error().startswith("svt_wav_parse")
    rc, got, _ = parse(data[:want["data_offset"]])   # the header alone: a file of no frames
    assert rc == OK and got == dict(want, frames=0)


def test_bad_arguments_are_refused():
    lib = _lib.load()
    data = GOOD["f32"][0]
    wi = _lib.WavInfoC(**PREFILL)
    need = ctypes.c_int64(-1)
    assert lib.svt_wav_parse(data, len(data), len(data), None, ctypes.byref(need)) == INVALID
    assert lib.svt_wav_parse(data, -1, len(data), ctypes.byref(wi), ctypes.byref(need)) == INVALID
    assert lib.svt_wav_parse(data, len(data), len(data) - 1, ctypes.byref(wi), ctypes.byref(need)) == INVALID
    assert lib.svt_wav_parse(None, 4, len(data), ctypes.byref(wi), ctypes.byref(need)) == INVALID
    assert lib.svt_wav_parse(data, 4, len(data), ctypes.byref(wi), None) == INVALID      # it would have to ask for more
    assert {f: getattr(wi, f) for f in FIELDS} == PREFILL
    assert lib.svt_wav_parse(data, len(data), len(data), ctypes.byref(wi), None) == OK    # nothing to ask for


def header(fmt, channels, rate, frames, capacity=64):
    lib = _lib.load()
    buf = ctypes.create_string_buffer(b"\xEE" * max(capacity, 1), max(capacity, 1))
    n = ctypes.c_int64(-1)
    rc = lib.svt_wav_header(fmt, channels, rate, frames, buf, capacity, ctypes.byref(n))
    return rc, buf.raw, n.value


@pytest.mark.parametrize("fmt,size", ((WC.S16, 44), (WC.F32, 58)))
def test_header_round_trip(fmt, size):
    for channels in range(1, 9):
        for rate, frames in ((16000, 0), (44100, 12345), (1, 1), (2 ** 31 - 1, 77)):
            rc, raw, n = header(fmt, channels, rate, frames, capacity=size)   # an exact-size buffer
            assert rc == OK and n == size, _lib.last_error()
            align = channels * WC.BYTES[fmt]
            rc, got, _ = parse(raw[:size], file_bytes=size + frames * align)
            assert rc == OK, _lib.last_error()
            assert got == WC.expect(fmt, channels, rate, size, frames)
    # the largest file that fits, and one frame more
    most = (0xFFFFFFFF - size) // (2 * WC.BYTES[fmt])
    rc, raw, n = header(fmt, 2, 48000, most)
    assert rc == OK and parse(raw[:n], file_bytes=n + most * 2 * WC.BYTES[fmt])[1]["frames"] == most
    assert header(fmt, 2, 48000, most + 1)[0] == INVALID and _lib.last_error().startswith("svt_wav_header")


def test_header_layout():
    rc, raw, n = header(WC.S16, 2, 44100, 10)
    assert n == 44 and raw[4:8] == (36 + 40).to_bytes(4, "little")
    assert raw[:4] == b"RIFF" and raw[8:16] == b"WAVEfmt " and raw[36:40] == b"data" and raw[40:44] == (40).to_bytes(4, "little")
    assert raw[12:36] == WC.fmt16(1, 2, 44100, 16)
    rc, raw, n = header(WC.F32, 3, 16000, 10)
    assert n == 58 and raw[12:38] == WC.fmt18(3, 3, 16000, 32)
    assert raw[38:50] == WC.chunk(b"fact", (10).to_bytes(4, "little")) and raw[50:58] == b"data" + (120).to_bytes(4, "little")
    assert raw[4:8] == (50 + 120).to_bytes(4, "little") and raw[58:] == b"\xEE" * 6


def test_header_refusals():
    for args in ((WC.S24, 2, 44100, 10), (WC.F64, 2, 44100, 10), (0, 2, 44100, 10), (WC.S16, 0, 44100, 10), (WC.S16, 9, 44100, 10),
                 (WC.S16, 2, 0, 10), (WC.S16, 2, 44100, -1)):
        rc, raw, n = header(*args)
        assert rc == INVALID and raw == b"\xEE" * 64 and n == -1, args
        assert _lib.last_error().startswith("svt_wav_header")
    assert header(WC.S16, 2, 44100, 10, capacity=43)[0] == INVALID
    assert header(WC.F32, 2, 44100, 10, capacity=57)[0] == INVALID


@pytest.mark.parametrize("channels", (1, 2, 3))
def test_the_wave_module_reads_our_16_bit_files(channels):
    frames = 9
    body = WC.payload(frames * channels * 2, 40 + channels)
    rc, raw, n = header(WC.S16, channels, 32000, frames)
    with wave.open(io.BytesIO(raw[:n] + body), "rb") as w:
        p = w.getparams()
        assert (p.nchannels, p.sampwidth, p.framerate, p.nframes) == (channels, 2, 32000, frames)
        assert w.readframes(frames) == body


# scipy takes a data size of 0 literally (no frames) and raises on a trailing partial frame; the parser here reads the first to the end of
# the file and drops the second, as libsndfile-based readers do.  On every other file the two must agree.
SCIPY_DIFFERS = {"size_zero", "partial_frame_open", "partial_frame"}


@pytest.mark.parametrize("name", sorted(set(GOOD) - SCIPY_DIFFERS))
def test_scipy_agrees(name):
    wavfile = pytest.importorskip("scipy.io.wavfile")
    import warnings
    data, want = GOOD[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # "chunk not understood" for LIST / JUNK, "reached EOF prematurely" for the overlong data size
        rate, arr = wavfile.read(io.BytesIO(data))
    assert rate == want["sample_rate"]
    arr = arr.reshape(want["frames"], want["channels"])
    raw = data[want["data_offset"]:want["data_offset"] + want["frames"] * want["block_align"]]
    ours = WC.decode_np(raw, want["format"], want["channels"]).T
    fmt = want["format"]
    if fmt == WC.U8:
        assert arr.dtype == np.uint8 and np.array_equal((arr.astype(np.float64) - 128) / 128, ours.astype(np.float64))
    elif fmt == WC.S16:
        assert arr.dtype == np.int16 and np.array_equal(arr.astype(np.float64) / 2.0 ** 15, ours.astype(np.float64))
    elif fmt == WC.S24:     # scipy: int32, left-shifted by 8
        assert arr.dtype == np.int32 and not (arr & 0xFF).any() and np.array_equal(arr.astype(np.float64) / 2.0 ** 31, ours.astype(np.float64))
    elif fmt == WC.S32:
        assert arr.dtype == np.int32 and np.array_equal((arr.astype(np.float64) / 2.0 ** 31).astype(np.float32).view(np.int32), ours.view(np.int32))
    elif fmt == WC.F32:
        assert arr.dtype == np.float32 and np.array_equal(arr.view(np.int32), ours.view(np.int32))
    else:
        assert arr.dtype == np.float64
        with np.errstate(all="ignore"):
            want32 = arr.astype(np.float32)
        assert np.array_equal(want32.view(np.int32)[~np.isnan(want32)], ours.view(np.int32)[~np.isnan(want32)])


def test_the_numpy_identities_behind_the_expected_values():
    """int32 -> float32 then an exact scale equals one rounding of x / 2^31, on the ties and the ends; rint in float64 is the S16 rule."""
    t = [(1 << 24) + 1, (1 << 24) + 3, (1 << 25) + 2, (1 << 25) + 6]
    x = np.array([-(1 << 31), (1 << 31) - 1, -1, 0, 1] + t + [-v for v in t], dtype=np.int32)
    a = x.astype(np.float32) * np.float32(2.0 ** -31)
    b = (x.astype(np.float64) / 2.0 ** 31).astype(np.float32)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert a[1] == np.float32(1.0) and a[0] == np.float32(-1.0)
    assert np.array_equal(x[5:9].astype(np.float32), np.array([1 << 24, (1 << 24) + 4, 1 << 25, (1 << 25) + 8], dtype=np.float32))
    q = WC.encode_s16_np(np.array([0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768, 1.0, -1.0, 32767.5 / 32768, -32768.5 / 32768,
                                   2.0, np.nan, np.inf, -np.inf, 1e-40], dtype=np.float32))
    assert q.tolist() == [0, 2, 2, 0, -2, 32767, -32768, 32767, -32768, 32767, 0, 32767, -32768, 0]
