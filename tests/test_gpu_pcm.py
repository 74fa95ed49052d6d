"""svt_pcm_decode / svt_pcm_encode on the GPU (csrc/pcm.hip) through the C ABI.  Every comparison is exact, on integer views of the whole
destination buffer: the expected buffer holds the numpy conversion (tests/wav_cases.py) where the call may write and a poison pattern
everywhere else -- guards in front of the first row and behind the last, the gaps of a padded pitch -- so one comparison checks values
and bounds alike.  The source sits at every byte offset behind a fresh allocation, the destination at every float (decode) or byte
(encode) offset.

A lane converts a group of 4, 8 or 16 frames (block_align a multiple of 4, even, odd) with vector accesses; the first group of a
misaligned buffer and whatever does not fill a group at the end go byte by byte.  Lengths: 1, 3 (no group), 4, 5 (one group of the wide
formats and a frame), 63 / 64 / 65 (several groups, with and without a rest, for every group size), 1027 and 4099 (beyond one workgroup's
4096 frames: a second tile), and one call a few frames beyond SVT_PCM_FRAMES_PER_WORKGROUP * SVT_PCM_MAX_WORKGROUPS, where the grid-stride
loop takes its second trip."""
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import wav_cases as WC  # noqa: E402
from svt_speechbrain_amd import _lib, audio_io  # noqa: E402

DEV = "cuda:0"
POISON = 0x7FC0DEAD      # a NaN with a payload: a write of any value, NaN included, changes the bits
POISON_BYTE = 0xA5
GUARD = 64
INVALID = -1
FORMATS = (WC.U8, WC.S16, WC.S24, WC.S32, WC.F32, WC.F64)
NAMES = {WC.U8: "U8", WC.S16: "S16", WC.S24: "S24", WC.S32: "S32", WC.F32: "F32", WC.F64: "F64"}
LENGTHS = (1, 3, 4, 5, 63, 64, 65, 1027, 4099)
SRC_OFFSETS = {f: tuple(range(16)) if f in (WC.S24, WC.U8) else (0, 1, 2, 3, 5, 8, 13) for f in FORMATS}


def test_the_exported_constants_are_the_headers():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svt_mi355.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define (SVT_PCM_[A-Z_]+) (\d+)", hdr)}
    assert got == {"SVT_PCM_FRAMES_PER_WORKGROUP": audio_io.FRAMES_PER_WORKGROUP, "SVT_PCM_MAX_WORKGROUPS": audio_io.MAX_WORKGROUPS}


_cache = {}


def case(fmt, channels, frames):
    """(raw interleaved bytes as uint8, expected (C, n) float32) of a format, a channel count and a length: computed once, never changed."""
    key = (fmt, channels, frames)
    if key not in _cache:
        raw = np.frombuffer(WC.interleave(WC.samples(fmt, channels, frames, 7 * frames + channels), fmt), dtype=np.uint8)
        assert raw.size == frames * channels * WC.BYTES[fmt]
        _cache[key] = (raw, WC.decode_np(raw.tobytes(), fmt, channels))
    return _cache[key]


def place_src(raw, off):
    """raw bytes `off` bytes behind the start of a fresh allocation plus GUARD; the rest poison.  -> (buffer, device address)"""
    buf = torch.full((GUARD + 16 + raw.size + GUARD,), POISON_BYTE, dtype=torch.uint8, device=DEV)
    buf[GUARD + off:GUARD + off + raw.size] = torch.from_numpy(raw.copy()).to(DEV)
    return buf, _lib.ptr(buf) + GUARD + off


def decode(raw, fmt, channels, frames, src_off=0, out_off=0, pad=0, downmix=False, expect=0, over=None):
    """One svt_pcm_decode call; over: arguments passed instead of the true ones (the refusals).  -> (the whole destination buffer as
    int32 on the host, the index of its first row's first element, ld_out, rows)"""
    lib = _lib.load()
    src, src_ptr = place_src(raw, src_off)
    rows = 1 if downmix else channels
    ld = frames + pad
    out = torch.full((GUARD + out_off + rows * ld + GUARD,), POISON, dtype=torch.int32, device=DEV)
    lo = GUARD + out_off
    a = dict(src=src_ptr, format=fmt, channels=channels, frames=frames, out=_lib.ptr(out) + 4 * lo, ld=ld, downmix=int(downmix))
    a.update(over or {})
    rc = lib.svt_pcm_decode(a["src"], a["format"], a["channels"], a["frames"], a["out"], a["ld"], a["downmix"], 0, _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == expect, (rc, _lib.last_error())
    return out.cpu().numpy(), lo, ld, rows


def expected_buffer(size, lo, ld, want):
    buf = np.full(size, POISON, dtype=np.int32)
    for r in range(want.shape[0]):
        buf[lo + r * ld:lo + r * ld + want.shape[1]] = want[r].view(np.int32)
    return buf


def same(got, want_buf, nan_ok=False):
    """Bit for bit; with nan_ok an expected NaN (other than the poison) is matched by any NaN."""
    if nan_ok:
        nan = np.isnan(want_buf.view(np.float32)) & (want_buf != POISON)
        if not np.isnan(got.view(np.float32)[nan]).all():
            return False
        got, want_buf = np.where(nan, 0, got), np.where(nan, 0, want_buf)
    return np.array_equal(got, want_buf)


def run_decode_offsets(fmt, channels, frames):
    raw, want = case(fmt, channels, frames)
    for k, src_off in enumerate(SRC_OFFSETS[fmt]):
        out_off, pad = k % 4, 5 * ((k // 4 + k) % 2)
        got, lo, ld, _ = decode(raw, fmt, channels, frames, src_off, out_off, pad)
        assert same(got, expected_buffer(got.size, lo, ld, want), nan_ok=fmt == WC.F64), (NAMES[fmt], channels, frames, src_off, out_off, pad)


@pytest.mark.parametrize("frames", LENGTHS)
@pytest.mark.parametrize("channels", (1, 2, 3))
@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_decode_every_format_at_every_source_offset(fmt, channels, frames):
    run_decode_offsets(fmt, channels, frames)


@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_decode_eight_channels(fmt):
    run_decode_offsets(fmt, 8, 65)


@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_the_special_values_are_in_the_cases(fmt):
    """The listed values lead every case that has room for them, and the numpy rule maps them where the issue says."""
    raw, want = case(fmt, 1, 63)
    sp = WC.special_values(fmt)
    assert np.array_equal(np.frombuffer(WC.interleave(sp[None, :], fmt), dtype=np.uint8), raw[:sp.size * WC.BYTES[fmt]])
    w = want[0, :sp.size]
    if fmt == WC.U8:
        assert w.tolist() == [-1.0, 127 / 128, -1 / 128, 0.0, 1 / 128, -127 / 128]
    elif fmt in (WC.S16, WC.S24):
        bits = 15 if fmt == WC.S16 else 23
        assert w.tolist() == [-1.0, 1 - 2.0 ** -bits, -2.0 ** -bits, 0.0, 2.0 ** -bits]
    elif fmt == WC.S32:
        assert w[:5].tolist() == [-1.0, 1.0, -2.0 ** -31, 0.0, 2.0 ** -31]
        assert (w[5:9] * 2.0 ** 31).tolist() == [1 << 24, (1 << 24) + 4, 1 << 25, (1 << 25) + 8]
    elif fmt == WC.F32:
        assert np.array_equal(w.view(np.uint32), sp)
    else:
        assert w[:3].tolist() == [1.0, 1 + 2.0 ** -22, -1.0] and w[3] == np.float32(1 + 2.0 ** -23)
        assert w[4:10].tolist() == [0.0, -0.0, 0.0, 2.0 ** -149, 2.0 ** -149, 3 * 2.0 ** -140] and np.signbit(w[5])
        assert w[10] == 0.0 and np.isinf(w[11:15]).all() and np.isnan(w[15]) and np.isinf(w[18])


@pytest.mark.parametrize("frames", LENGTHS)
@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_downmix(fmt, frames):
    raw, want = case(fmt, 2, frames)
    with np.errstate(invalid="ignore", over="ignore"):
        mono = (np.float32(0.5) * (want[0] + want[1]))[None, :]
    assert mono.dtype == np.float32
    for k, src_off in enumerate((0, 1, 2, 3, 6, 13)):
        got, lo, ld, _ = decode(raw, fmt, 2, frames, src_off, k % 4, 5 * (k % 2), downmix=True)
        assert same(got, expected_buffer(got.size, lo, ld, mono), nan_ok=True), (NAMES[fmt], frames, src_off)


def test_beyond_the_grid_cap():
    frames = audio_io.FRAMES_PER_WORKGROUP * audio_io.MAX_WORKGROUPS + 5
    rng = np.random.RandomState(3)
    raw = rng.randint(0, 256, 2 * frames, dtype=np.int64).astype(np.uint8)
    want = WC.decode_np(raw.tobytes(), WC.S16, 1)
    for src_off in (0, 1):
        got, lo, ld, _ = decode(raw, WC.S16, 1, frames, src_off, 1, 0)
        assert same(got, expected_buffer(got.size, lo, ld, want)), src_off


def test_decode_refusals_leave_the_destination_untouched():
    raw, _ = case(WC.S16, 2, 64)
    bad = [dict(out=0), dict(src=0), dict(channels=0), dict(channels=9), dict(frames=0), dict(frames=-3), dict(ld=63), dict(format=0),
           dict(format=7), dict(downmix=1, channels=1), dict(downmix=1, channels=3)]
    for over in bad:
        got, *_ = decode(raw, WC.S16, 2, 64, expect=INVALID, over=over)
        assert (got == POISON).all(), over
        assert _lib.last_error().startswith("svt_pcm_decode"), (over, _lib.last_error())
    lib = _lib.load()
    out = torch.full((GUARD + 2 * 64 + GUARD,), POISON, dtype=torch.int32, device=DEV)
    src, src_ptr = place_src(raw, 0)
    for off in (1, 2, 3):   # a misaligned destination
        assert lib.svt_pcm_decode(src_ptr, WC.S16, 2, 64, _lib.ptr(out) + 4 * GUARD + off, 64, 0, 0, _lib.stream_ptr(DEV)) == INVALID
        assert _lib.last_error().startswith("svt_pcm_decode")
    torch.cuda.synchronize()
    assert bool((out == POISON).all())


# ---- encode ----

def encode_inputs(fmt, channels, frames):
    """(C, n) float32: for S16 the ties of both parities, the ends of the range and what lies beyond, NaN, infinities and denormals first;
    for F32 the bit patterns of the decode case."""
    key = ("enc", fmt, channels, frames)
    if key not in _cache:
        n = channels * frames
        if fmt == WC.F32:
            x = WC.samples(WC.F32, channels, frames, 5 * frames + channels).view(np.float32)
        else:
            rng = np.random.RandomState(11 * frames + channels)
            v = rng.uniform(-1.1, 1.1, n).astype(np.float32)
            sp = np.array([0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768, -2.5 / 32768, 12344.5 / 32768, 12345.5 / 32768,
                           1.0, -1.0, 32767.5 / 32768, -32768.5 / 32768, 32766.5 / 32768, 2.0, -2.0, np.nan, np.inf, -np.inf, 1e-40, -1e-40,
                           np.float32(2.0 ** -149), 0.0, -0.0, 0.49999997 / 32768], dtype=np.float32)
            k = min(sp.size, n)
            v[:k] = sp[:k]
            x = v.reshape(frames, channels).T.copy()
        _cache[key] = x
    return _cache[key]


def encoded_bytes(x, fmt):
    if fmt == WC.F32:
        return np.frombuffer(np.ascontiguousarray(x.T).view(np.uint32).astype("<u4").tobytes(), dtype=np.uint8)
    return np.frombuffer(np.ascontiguousarray(WC.encode_s16_np(x).T).astype("<i2").tobytes(), dtype=np.uint8)


def encode(x, fmt, in_off=0, pad=0, dst_off=0, expect=0, over=None):
    """One svt_pcm_encode call.  -> (the whole destination buffer as uint8 on the host, the index of the first byte)"""
    lib = _lib.load()
    channels, frames = x.shape
    ld = frames + pad
    src = torch.full((GUARD + in_off + channels * ld + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    src[GUARD + in_off:GUARD + in_off + channels * ld].view(channels, ld)[:, :frames] = torch.from_numpy(x.copy()).to(DEV)
    nbytes = frames * channels * WC.BYTES[fmt]
    dst = torch.full((GUARD + 8 + nbytes + GUARD,), POISON_BYTE, dtype=torch.uint8, device=DEV)
    lo = GUARD + dst_off
    a = dict(src=_lib.ptr(src) + 4 * (GUARD + in_off), ld=ld, channels=channels, frames=frames, format=fmt, dst=_lib.ptr(dst) + lo)
    a.update(over or {})
    rc = lib.svt_pcm_encode(a["src"], a["ld"], a["channels"], a["frames"], a["format"], a["dst"], 0, _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == expect, (rc, _lib.last_error())
    return dst.cpu().numpy(), lo


def run_encode_offsets(fmt, channels, frames):
    x = encode_inputs(fmt, channels, frames)
    want = encoded_bytes(x, fmt)
    for dst_off in range(8):
        in_off, pad = (dst_off + 1) % 4, 5 * ((dst_off // 2) % 2)
        got, lo = encode(x, fmt, in_off, pad, dst_off)
        buf = np.full(got.size, POISON_BYTE, dtype=np.uint8)
        buf[lo:lo + want.size] = want
        assert np.array_equal(got, buf), (NAMES[fmt], channels, frames, dst_off, in_off, pad)


@pytest.mark.parametrize("frames", LENGTHS)
@pytest.mark.parametrize("channels", (1, 2, 3))
@pytest.mark.parametrize("fmt", (WC.S16, WC.F32), ids=NAMES.get)
def test_encode_at_every_destination_offset(fmt, channels, frames):
    run_encode_offsets(fmt, channels, frames)


@pytest.mark.parametrize("fmt", (WC.S16, WC.F32), ids=NAMES.get)
def test_encode_eight_channels(fmt):
    run_encode_offsets(fmt, 8, 65)


def test_the_s16_rule_on_its_special_inputs():
    x = encode_inputs(WC.S16, 1, 63)
    assert WC.encode_s16_np(x)[0, :24].tolist() == [0, 2, 2, 0, -2, -2, 12344, 12346, 32767, -32768, 32767, -32768, 32766, 32767, -32768, 0,
                                                     32767, -32768, 0, 0, 0, 0, 0, 0]


def test_encode_refusals_leave_the_destination_untouched():
    x = encode_inputs(WC.S16, 2, 64)
    for over in (dict(src=0), dict(dst=0), dict(channels=0), dict(channels=9), dict(frames=0), dict(ld=63), dict(format=WC.S24),
                 dict(format=WC.U8), dict(format=WC.F64), dict(format=0)):
        got, _ = encode(x, WC.S16, expect=INVALID, over=over)
        assert (got == POISON_BYTE).all(), over
        assert _lib.last_error().startswith("svt_pcm_encode"), (over, _lib.last_error())
    src = torch.zeros(256, dtype=torch.float32, device=DEV)
    dst = torch.full((1024,), POISON_BYTE, dtype=torch.uint8, device=DEV)
    assert _lib.load().svt_pcm_encode(_lib.ptr(src) + 2, 64, 2, 64, WC.S16, _lib.ptr(dst), 0, _lib.stream_ptr(DEV)) == INVALID
    torch.cuda.synchronize()
    assert bool((dst == POISON_BYTE).all())


def test_encode_then_decode_reproduces_any_s16_source():
    """decode(encode_S16(decode(s))) == decode(s), and the encoded bytes are s itself: x / 2^15 * 32768 is exact."""
    lib = _lib.load()
    frames, channels = 4099, 2
    raw, want = case(WC.S16, channels, frames)
    src, src_ptr = place_src(raw, 3)
    x = torch.empty((channels, frames), dtype=torch.float32, device=DEV)
    back = torch.empty(raw.size + 1, dtype=torch.uint8, device=DEV)
    st = _lib.stream_ptr(DEV)
    assert lib.svt_pcm_decode(src_ptr, WC.S16, channels, frames, _lib.ptr(x), frames, 0, 0, st) == 0
    assert lib.svt_pcm_encode(_lib.ptr(x), frames, channels, frames, WC.S16, _lib.ptr(back) + 1, 0, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(back.cpu().numpy()[1:], raw)
    assert np.array_equal(x.cpu().numpy().view(np.int32), want.view(np.int32))


def test_two_calls_give_the_same_bytes():
    raw, _ = case(WC.S24, 2, 4099)
    a = decode(raw, WC.S24, 2, 4099, 5, 1, 5)[0]
    b = decode(raw, WC.S24, 2, 4099, 5, 1, 5)[0]
    assert np.array_equal(a, b)
    x = encode_inputs(WC.S16, 2, 4099)
    assert np.array_equal(encode(x, WC.S16, 1, 5, 3)[0], encode(x, WC.S16, 1, 5, 3)[0])


def test_decode_and_encode_captured_in_a_graph_replay_bit_identically():
    """The header promises that neither call synchronises or allocates: both are captured into one graph and replayed on new input."""
    lib = _lib.load()
    frames, channels = 4099, 2
    raw_a, want_a = case(WC.S24, channels, frames)
    raw_b = np.roll(raw_a, 6 * 17)
    want_b = WC.decode_np(raw_b.tobytes(), WC.S24, channels)
    src = torch.zeros(raw_a.size + 16, dtype=torch.uint8, device=DEV)
    x = torch.zeros((channels, frames), dtype=torch.float32, device=DEV)
    pcm = torch.zeros(frames * channels * 2 + 16, dtype=torch.uint8, device=DEV)

    def call():
        st = _lib.stream_ptr(DEV)
        _lib.check(lib.svt_pcm_decode(_lib.ptr(src) + 6, WC.S24, channels, frames, _lib.ptr(x), frames, 0, 0, st), "svt_pcm_decode")
        _lib.check(lib.svt_pcm_encode(_lib.ptr(x), frames, channels, frames, WC.S16, _lib.ptr(pcm) + 2, 0, st), "svt_pcm_encode")

    src[6:6 + raw_a.size] = torch.from_numpy(raw_a.copy()).to(DEV)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                             # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        call()
    x.zero_(); pcm.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy().view(np.int32), want_a.view(np.int32))
    assert np.array_equal(pcm.cpu().numpy()[2:2 + 4 * frames], encoded_bytes(want_a, WC.S16))
    src[6:6 + raw_b.size] = torch.from_numpy(raw_b.copy()).to(DEV)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy().view(np.int32), want_b.view(np.int32))
    assert np.array_equal(pcm.cpu().numpy()[2:2 + 4 * frames], encoded_bytes(want_b, WC.S16))
