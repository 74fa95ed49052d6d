"""Shared by the wav tests (test_wav_host.py, test_wav_sanitizers.py, test_gpu_pcm.py, test_gpu_audio_io.py): RIFF/WAVE files built byte
by byte or by the stdlib ``wave`` module, what a correct parser reads from each, the files a parser must refuse, and the numpy side of the
sample conversion.  Nothing here calls the code under test."""
import io
import struct
import wave

import numpy as np

U8, S16, S24, S32, F32, F64 = 1, 2, 3, 4, 5, 6
BYTES = {U8: 1, S16: 2, S24: 3, S32: 4, F32: 4, F64: 8}
GUID_TAIL = bytes([0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71])


def chunk(cid, payload, size=None):
    """One chunk: id, size (the payload's, unless overridden), payload, the pad byte after an odd payload."""
    return cid + struct.pack("<I", len(payload) if size is None else size) + payload + (b"\0" if len(payload) & 1 else b"")


def riff(*chunks, magic=b"RIFF", form=b"WAVE"):
    body = form + b"".join(chunks)
    return magic + struct.pack("<I", len(body)) + body


def fmt16(tag, channels, rate, bits, align=None):
    align = channels * bits // 8 if align is None else align
    return chunk(b"fmt ", struct.pack("<HHIIHH", tag, channels, rate, rate * align & 0xFFFFFFFF, align, bits))


def fmt18(tag, channels, rate, bits):
    align = channels * bits // 8
    return chunk(b"fmt ", struct.pack("<HHIIHHH", tag, channels, rate, rate * align, align, bits, 0))


def fmt_ext(sub_tag, channels, rate, bits, valid=None, tail=GUID_TAIL):
    align = channels * bits // 8
    return chunk(b"fmt ", struct.pack("<HHIIHHHHI", 0xFFFE, channels, rate, rate * align, align, bits, 22, bits if valid is None else valid,
                                      (1 << channels) - 1) + struct.pack("<H", sub_tag) + tail)


def payload(n_bytes, seed):
    return np.random.RandomState(seed).randint(0, 256, n_bytes, dtype=np.uint8).tobytes()


def expect(fmt, channels, rate, data_offset, frames):
    bits = 8 * BYTES[fmt]
    return dict(format=fmt, channels=channels, sample_rate=rate, bits_per_sample=bits, block_align=channels * bits // 8,
                data_offset=data_offset, frames=frames)


def wave_module_file(width, channels, frames=7, rate=22050):
    """(bytes, params) of a file the stdlib writes: sample width 1..4 bytes."""
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(payload(frames * channels * width, 10 * width + channels))
    return buf.getvalue()


def well_formed():
    """name -> (file bytes, what svt_wav_parse must return)."""
    out = {}
    for width, fmt in ((1, U8), (2, S16), (3, S24), (4, S32)):
        for channels in (1, 2, 3):
            out[f"wave_w{width}_c{channels}"] = (wave_module_file(width, channels), expect(fmt, channels, 22050, 44, 7))
    d = payload(5 * 2 * 4, 1)
    out["f32"] = (riff(fmt18(3, 2, 44100, 32), chunk(b"data", d)), expect(F32, 2, 44100, 46, 5))
    d = payload(3 * 1 * 8, 2)
    out["f64"] = (riff(fmt18(3, 1, 8000, 64), chunk(b"data", d)), expect(F64, 1, 8000, 46, 3))
    d = payload(4 * 2 * 2, 3)
    out["ext_pcm"] = (riff(fmt_ext(1, 2, 48000, 16), chunk(b"data", d)), expect(S16, 2, 48000, 68, 4))
    d = payload(4 * 3 * 4, 4)
    out["ext_float"] = (riff(fmt_ext(3, 3, 96000, 32), chunk(b"data", d)), expect(F32, 3, 96000, 68, 4))
    d = payload(6 * 2, 5)
    out["odd_list"] = (riff(fmt16(1, 1, 16000, 16), chunk(b"LIST", b"INFOabc"), chunk(b"data", d)), expect(S16, 1, 16000, 36 + 16 + 8, 6))
    out["list_first"] = (riff(chunk(b"JUNK", b"\0" * 11), fmt16(1, 1, 16000, 16), chunk(b"data", d)), expect(S16, 1, 16000, 12 + 20 + 24 + 8, 6))
    d = payload(6 * 4, 6)
    out["fact"] = (riff(fmt18(3, 1, 16000, 32), chunk(b"fact", struct.pack("<I", 6)), chunk(b"data", d)), expect(F32, 1, 16000, 58, 6))
    d = payload(5 * 3, 7)   # an odd data size: the pad byte, then a chunk behind it
    out["chunk_after"] = (riff(fmt16(1, 1, 11025, 24), chunk(b"data", d), chunk(b"LIST", b"INFOxy")), expect(S24, 1, 11025, 44, 5))
    d = payload(9 * 4, 8)
    for name, size in (("size_zero", 0), ("size_ffff", 0xFFFFFFFF), ("size_past_end", len(d) + 100)):
        out[name] = (riff(fmt16(1, 2, 44100, 16), chunk(b"data", d, size=size)), expect(S16, 2, 44100, 44, 9))
    out["partial_frame"] = (riff(fmt16(1, 2, 44100, 24), chunk(b"data", payload(6 * 4 + 5, 9))), expect(S24, 2, 44100, 44, 4))
    out["partial_frame_open"] = (riff(fmt16(1, 2, 44100, 16), chunk(b"data", payload(4 * 3 + 2, 9), size=0)), expect(S16, 2, 44100, 44, 3))
    return out


def refused():
    """name -> file bytes a parser must refuse, whole: none of them is merely a short prefix."""
    d = chunk(b"data", payload(16, 20))
    good = fmt16(1, 2, 44100, 16)
    out = {
        "rifx": riff(good, d, magic=b"RIFX"),
        "rf64": riff(good, d, magic=b"RF64"),
        "w64": b"riff" + bytes([0x2E, 0x91, 0xCF, 0x11, 0xA5, 0xD6, 0x28, 0xDB, 0x04, 0xC1, 0x00, 0x00]) + payload(64, 21),
        "not_wave": riff(good, d, form=b"AVI "),
        "alaw": riff(fmt18(6, 1, 8000, 8), d),
        "mulaw": riff(fmt18(7, 1, 8000, 8), d),
        "adpcm": riff(fmt18(2, 1, 8000, 4), d),
        "ima_adpcm": riff(fmt18(0x11, 1, 8000, 4), d),
        "mp3_tag": riff(fmt18(0x55, 2, 44100, 16), d),
        "data_before_fmt": riff(d, good),
        "no_fmt": riff(d),
        "zero_channels": riff(fmt16(1, 0, 44100, 16), d),
        "nine_channels": riff(fmt16(1, 9, 44100, 16), d),
        "zero_rate": riff(fmt16(1, 2, 0, 16), d),
        "bad_block_align": riff(fmt16(1, 2, 44100, 16, align=6), d),
        "bits_12": riff(fmt16(1, 1, 44100, 12, align=2), d),
        "float_16": riff(fmt18(3, 1, 44100, 16), d),
        "pcm_64": riff(fmt16(1, 1, 44100, 64), d),
        "ext_guid": riff(fmt_ext(1, 2, 48000, 16, tail=GUID_TAIL[:-1] + b"\x72"), d),
        "ext_valid_bits": riff(fmt_ext(1, 2, 48000, 32, valid=24), d),
        "ext_sub_alaw": riff(fmt_ext(6, 1, 8000, 8), d),
        "short_fmt": riff(chunk(b"fmt ", struct.pack("<HHIIH", 1, 2, 44100, 176400, 4)), d),
        "empty": b"",
        "riff_only": b"RIFF\x04\0\0\0WAV",
        "cut_in_fmt": riff(good, d)[:30],
        "cut_before_data": riff(good, d)[:36],
        "cut_in_data_header": riff(good, d)[:41],
        "chunk_past_end": riff(good, chunk(b"LIST", b"INFOabcd", size=4000)),
        "no_data": riff(good, chunk(b"LIST", b"INFOabcd")),
    }
    return out


def interleave(samples, fmt):
    """(C, n) array of sample values in the format's own type (uint8 / int16 / int32 in 24 bits / int32 / float32 / float64, or float32
    given as uint32 bits) -> the little-endian interleaved bytes of a data chunk."""
    a = np.ascontiguousarray(np.asarray(samples).T)
    if fmt == S24:
        b = a.astype("<i4").view(np.uint8).reshape(a.shape + (4,))[..., :3]
        return np.ascontiguousarray(b).tobytes()
    dt = {U8: "u1", S16: "<i2", S32: "<i4", F32: "<u4" if a.dtype == np.uint32 else "<f4", F64: "<f8"}[fmt]
    return a.astype(dt).tobytes()


def decode_np(raw, fmt, channels):
    """The value rule in numpy: interleaved bytes -> (C, n) float32.  Every step is exact except the int32 -> float32 and float64 ->
    float32 conversions, which round to nearest, ties to even, once."""
    b = np.frombuffer(raw, dtype=np.uint8)
    if fmt == U8:
        x = (b.astype(np.float32) - np.float32(128)) * np.float32(2.0 ** -7)
    elif fmt == S16:
        x = b.view("<i2").astype(np.float32) * np.float32(2.0 ** -15)
    elif fmt == S24:
        t = b.reshape(-1, 3).astype(np.int32)
        v = t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        x = v.astype(np.float32) * np.float32(2.0 ** -23)
    elif fmt == S32:
        x = b.view("<i4").astype(np.float32) * np.float32(2.0 ** -31)
    elif fmt == F32:
        x = b.view("<f4")
    else:
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            x = b.view("<f8").astype(np.float32)
    return np.ascontiguousarray(x.reshape(-1, channels).T)


def encode_s16_np(x):
    """q = clamp(rint(x * 32768), -32768, 32767), ties to even, NaN -> 0, in float64 (the product is exact there)."""
    with np.errstate(invalid="ignore"):
        y = np.rint(np.asarray(x, dtype=np.float32).astype(np.float64) * 32768.0)
    y = np.where(np.isnan(y), 0.0, np.clip(y, -32768.0, 32767.0))
    return y.astype(np.int16)


def wav_file(fmt, channels, rate, raw):
    """A plain file around a data chunk: 16-byte fmt for PCM, 18-byte fmt and a fact chunk for float."""
    frames = len(raw) // (channels * BYTES[fmt])
    if fmt in (F32, F64):
        return riff(fmt18(3, channels, rate, 8 * BYTES[fmt]), chunk(b"fact", struct.pack("<I", frames)), chunk(b"data", raw))
    return riff(fmt16(1, channels, rate, 8 * BYTES[fmt]), chunk(b"data", raw))


def special_values(fmt):
    """The sample values the issue names, in the format's own numpy type (F32: uint32 bit patterns)."""
    if fmt == U8:
        return np.array([0, 255, 127, 128, 129, 1], dtype=np.uint8)
    if fmt == S16:
        return np.array([-32768, 32767, -1, 0, 1], dtype=np.int16)
    if fmt == S24:
        return np.array([-(1 << 23), (1 << 23) - 1, -1, 0, 1], dtype=np.int32)
    if fmt == S32:
        t = [(1 << 24) + 1, (1 << 24) + 3, (1 << 25) + 2, (1 << 25) + 6]
        return np.array([-(1 << 31), (1 << 31) - 1, -1, 0, 1] + t + [-v for v in t], dtype=np.int32)
    if fmt == F32:
        return np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x7FBFFFFF, 0x80000000, 0x00000000, 0x00000001, 0x80000001, 0x7F800000,
                         0xFF800000, 0x3F800000], dtype=np.uint32)
    one = np.float64(1.0)
    return np.array([one + 2.0 ** -24, one + 3 * 2.0 ** -24, -(one + 2.0 ** -24), one + 2.0 ** -24 + 2.0 ** -50, 2.0 ** -150, -2.0 ** -150,
                     2.0 ** -151, 1.5 * 2.0 ** -150, 2.0 ** -149, 3 * 2.0 ** -140, 1e-320, 1e300, -1e300, np.inf, -np.inf, np.nan, 0.0, -0.0,
                     3.4028235677973366e38], dtype=np.float64)


def samples(fmt, channels, frames, seed):
    """(C, n) values in the format's own type: the special values first (as many as fit), random after them."""
    rng = np.random.RandomState(seed)
    n = channels * frames
    if fmt == U8:
        v = rng.randint(0, 256, n).astype(np.uint8)
    elif fmt == S16:
        v = rng.randint(-32768, 32768, n).astype(np.int16)
    elif fmt == S24:
        v = rng.randint(-(1 << 23), 1 << 23, n).astype(np.int32)
    elif fmt == S32:
        v = rng.randint(-(1 << 31), 1 << 31, n, dtype=np.int64).astype(np.int32)
    elif fmt == F32:
        v = rng.uniform(-1, 1, n).astype(np.float32).view(np.uint32)
    else:
        v = rng.uniform(-1, 1, n)
    sp = special_values(fmt)
    k = min(len(sp), n)
    v[:k] = sp[:k]
    return v.reshape(frames, channels).T.copy()
