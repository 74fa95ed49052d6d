"""The Python layer over the wav parser and the PCM kernels (svt_speechbrain_amd/audio_io.py, dataio.read_utterance,
SongTranscriber.transcribe_file, NoiseSweep.run(write_wavs=True)) on the GPU, with files in tmp_path.  Expected samples come from the numpy
conversion of tests/wav_cases.py; every comparison is exact.  The bytes a load reads are counted by a file object put in the place of
audio_io's one way of opening a file, never by timing."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import wav_cases as WC  # noqa: E402
import svt_speechbrain_amd as S  # noqa: E402
from svt_speechbrain_amd import audio_io, dataio, weights as Wt  # noqa: E402
from svt_speechbrain_amd.config import PRESETS  # noqa: E402

DEV = "cuda:0"
FORMATS = (WC.U8, WC.S16, WC.S24, WC.S32, WC.F32, WC.F64)
NAMES = {WC.U8: "U8", WC.S16: "S16", WC.S24: "S24", WC.S32: "S32", WC.F32: "F32", WC.F64: "F64"}


def write_case(path, fmt, channels, frames, rate=22050, seed=1):
    """A wav file of seeded samples; -> the (C, n) float32 a correct load returns."""
    raw = WC.interleave(WC.samples(fmt, channels, frames, seed), fmt)
    path.write_bytes(WC.wav_file(fmt, channels, rate, raw))
    return WC.decode_np(raw, fmt, channels)


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def same(got, want, nan_ok=False):
    g, w = bits(got), want.view(np.int32)
    if g.shape != w.shape:
        return False
    if nan_ok:
        nan = np.isnan(want)
        if not np.isnan(g.view(np.float32)[nan]).all():
            return False
        g, w = np.where(nan, 0, g), np.where(nan, 0, w)
    return np.array_equal(g, w)


@pytest.mark.parametrize("channels", (1, 2, 3))
@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_load_equals_the_numpy_decode(tmp_path, fmt, channels):
    path = tmp_path / "a.wav"
    want = write_case(path, fmt, channels, 1027, rate=44100, seed=fmt + channels)
    meta = audio_io.info(str(path))
    assert tuple(meta) == (44100, 1027, channels, 8 * WC.BYTES[fmt], "PCM_U" if fmt == WC.U8 else "PCM_F" if fmt >= WC.F32 else "PCM_S")
    assert meta.sample_rate == 44100 and meta.num_frames == 1027 and meta.num_channels == channels
    got, fs = audio_io.load(str(path), device=DEV)
    assert fs == 44100 and got.dtype == torch.float32 and got.device == torch.device(DEV) and got.shape == (channels, 1027)
    assert same(got, want, nan_ok=fmt == WC.F64)
    flipped, _ = audio_io.load(path, channels_first=False, device=DEV)
    assert flipped.shape == (1027, channels) and same(flipped.t(), want, nan_ok=fmt == WC.F64)


class CountingFile:
    """A binary file that adds up the bytes handed out by read / readinto."""
    total = 0

    def __init__(self, path, mode):
        self.fh = open(path, mode)

    def read(self, n=-1):
        b = self.fh.read(n)
        CountingFile.total += len(b)
        return b

    def readinto(self, buf):
        n = self.fh.readinto(buf)
        CountingFile.total += n
        return n

    def seek(self, *a):
        return self.fh.seek(*a)

    def fileno(self):
        return self.fh.fileno()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.fh.close()


@pytest.mark.parametrize("fmt,channels", ((WC.S24, 2), (WC.S16, 1), (WC.F32, 3)), ids=("S24x2", "S16x1", "F32x3"))
def test_a_range_is_the_slice_of_the_whole_and_reads_only_its_bytes(tmp_path, monkeypatch, fmt, channels):
    frames = 30011
    path = tmp_path / "a.wav"
    want = write_case(path, fmt, channels, frames, seed=9)
    align = channels * WC.BYTES[fmt]
    whole, _ = audio_io.load(str(path), device=DEV)
    assert same(whole, want)
    monkeypatch.setattr(audio_io, "_open", CountingFile)
    for off, num, n in ((0, 5, 5), (0, 4097, 4097), (7, 1, 1), (12345, 8193, 8193), (frames - 100, 100, 100), (frames - 100, -1, 100),
                        (frames - 3, 50, 3), (frames, 10, 0), (frames + 77, -1, 0), (1, -1, frames - 1), (5, 0, 0)):
        CountingFile.total = 0
        got, _ = audio_io.load(str(path), frame_offset=off, num_frames=num, device=DEV)
        assert got.shape == (channels, n) and same(got, np.ascontiguousarray(want[:, off:off + n])), (off, num)
        assert CountingFile.total <= audio_io.HEADER_PREFIX + n * align, (off, num, CountingFile.total)
        assert CountingFile.total >= n * align


def test_read_audio_in_both_forms(tmp_path):
    mono, stereo = tmp_path / "m.wav", tmp_path / "s.wav"
    wm = write_case(mono, WC.S16, 1, 5003, rate=16000, seed=3)
    ws = write_case(stereo, WC.S24, 2, 5003, rate=16000, seed=4)
    a = S.read_audio(str(mono), DEV)
    assert a.shape == (5003,) and same(a, wm[0])
    b = S.read_audio(str(stereo), DEV)
    assert b.shape == (5003, 2) and same(b.t(), ws)
    c = S.read_audio({"file": str(mono), "start": 100, "stop": 2100}, DEV)
    assert c.shape == (2000,) and same(c, np.ascontiguousarray(wm[0, 100:2100]))
    d = S.read_audio({"file": str(stereo), "start": 4000}, DEV)     # no stop: to the end
    assert d.shape == (1003, 2) and same(d.t(), np.ascontiguousarray(ws[:, 4000:]))
    e = S.read_audio({"file": str(stereo), "start": 10, "stop": 12}, DEV)
    assert e.shape == (2, 2) and same(e.t(), np.ascontiguousarray(ws[:, 10:12]))


@pytest.mark.parametrize("seconds,utter_num,last", ((23, 5, 3000), (22, 4, 7000)))
def test_read_utterance_is_the_slice_of_the_whole_song(tmp_path, seconds, utter_num, last):
    """A 23 s file at 1 kHz: round(23 / 5) = 5 utterances, the last one 3 s; a 22 s one: round(22 / 5) = 4, the last one takes the
    remainder and is 7 s long."""
    rate, frames = 1000, seconds * 1000
    path = tmp_path / "song.wav"
    write_case(path, WC.S16, 1, frames, rate=rate, seed=5)
    whole = S.read_audio(str(path), DEV)
    assert utter_num == round(frames / rate / 5) == len(dataio.plan_utterances(seconds, 5))
    total = 0
    for utter_id in range(1, utter_num + 1):
        want = dataio.slice_audio(whole, utter_id, utter_num, sample_rate=rate, dur_threshold=5)
        got = S.read_utterance(str(path), utter_id, utter_num, sample_rate=rate, dur_threshold=5, device=DEV)
        assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32)), utter_id
        total += got.shape[0]
    assert total == frames and got.shape[0] == last


def test_save_then_load(tmp_path):
    rng = np.random.RandomState(12)
    for channels, frames in ((1, 1), (1, 4099), (2, 1027), (3, 65)):
        x = rng.uniform(-1.2, 1.2, (channels, frames)).astype(np.float32)
        x.flat[:6] = np.array([np.nan, -0.0, 1e-40, np.inf, 0.5 / 32768, 1.5 / 32768], dtype=np.float32)[:x.size]
        xd = torch.from_numpy(x).to(DEV)
        path = tmp_path / f"f_{channels}_{frames}.wav"
        audio_io.save(str(path), xd, 16000)
        meta = audio_io.info(str(path))
        assert tuple(meta) == (16000, frames, channels, 32, "PCM_F")
        assert path.stat().st_size == 58 + 4 * channels * frames
        assert path.read_bytes()[58:] == np.ascontiguousarray(x.T).tobytes()
        got, fs = audio_io.load(str(path), device=DEV)
        assert fs == 16000 and same(got, x)                              # the identity, NaN payloads included
        path = tmp_path / f"s_{channels}_{frames}.wav"
        audio_io.save(str(path), xd.t().contiguous(), 8000, channels_first=False, encoding="PCM_S", bits_per_sample=16)
        assert tuple(audio_io.info(str(path))) == (8000, frames, channels, 16, "PCM_S")
        q = WC.encode_s16_np(x)
        assert path.read_bytes()[44:] == np.ascontiguousarray(q.T).astype("<i2").tobytes()
        got, _ = audio_io.load(str(path), device=DEV)
        assert same(got, q.astype(np.float32) * np.float32(2.0 ** -15))
    # write_audio: speechbrain's (samples, channels), a float32 file
    y = torch.from_numpy(rng.uniform(-1, 1, (301, 2)).astype(np.float32)).to(DEV)
    S.write_audio(str(tmp_path / "w.wav"), y, 16000)
    assert torch.equal(S.read_audio(str(tmp_path / "w.wav"), DEV), y)
    S.write_audio(str(tmp_path / "w1.wav"), y[:, 0].contiguous(), 16000)
    assert torch.equal(S.read_audio(str(tmp_path / "w1.wav"), DEV), y[:, 0])
    with pytest.raises(ValueError):
        audio_io.save(str(tmp_path / "x.wav"), y.t(), 16000, encoding="PCM_S", bits_per_sample=24)


def test_back_to_back_loads_share_the_staging_buffer(tmp_path):
    """Two files of one size through the one pinned buffer, no synchronisation in between: each tensor holds its own file's samples."""
    frames = 200003
    a, b = tmp_path / "a.wav", tmp_path / "b.wav"
    wa = write_case(a, WC.S16, 2, frames, seed=21)
    wb = write_case(b, WC.S16, 2, frames, seed=22)
    assert not np.array_equal(wa, wb)
    for _ in range(3):
        ta, _ = audio_io.load(str(a), device=DEV)
        tb, _ = audio_io.load(str(b), device=DEV)
        tc, _ = audio_io.load(str(a), frame_offset=1, device=DEV)
        assert same(ta, wa) and same(tb, wb) and same(tc, np.ascontiguousarray(wa[:, 1:]))
    stage = audio_io._staging[torch.device(DEV)]
    assert stage.buf is not None and stage.buf.is_pinned() and stage.buf.numel() >= 4 * frames


def test_transcribe_file(tmp_path):
    """0.3 s of stereo 44.1 kHz 16-bit audio: transcribe_file is transcribe(load(...)[0], sample_rate=44100); a mono 16 kHz file goes
    straight to transcribe."""
    cfg = PRESETS["tiny-group"]
    hd = Wt.seeded_head_state_dict(cfg.hidden_size, 20, seed=32)
    enc = S.HuggingFaceWav2Vec2("tiny-group", None, config=cfg, precision="fp32", seed=31).to(DEV)
    head = S.Linear(20, input_size=cfg.hidden_size)
    head.load_state_dict(hd)
    head = head.to(DEV)
    tr = S.SongTranscriber(enc, head, sample_rate=16000, dur_threshold=0.25)
    path = tmp_path / "stereo.wav"
    rng = np.random.RandomState(77)
    pcm = (rng.uniform(-0.3, 0.3, (13230, 2)) * 32768).astype("<i2")
    path.write_bytes(WC.wav_file(WC.S16, 2, 44100, pcm.tobytes()))
    song, fs = S.load(str(path), device=DEV)
    assert fs == 44100 and song.shape == (2, 13230)
    want_notes, want_feats = tr.transcribe(song, return_feats=True, sample_rate=44100)
    notes, feats = tr.transcribe_file(str(path), return_feats=True, device=DEV)
    assert notes == want_notes and torch.equal(feats, want_feats)
    assert tr.transcribe_file(str(path), device=DEV) == want_notes
    mono = tmp_path / "mono.wav"
    m = (rng.uniform(-0.3, 0.3, 4800) * 32768).astype("<i2")
    mono.write_bytes(WC.wav_file(WC.S16, 1, 16000, m.tobytes()))
    want_notes, want_feats = tr.transcribe(S.load(str(mono), device=DEV)[0][0], return_feats=True)
    notes, feats = tr.transcribe_file(str(mono), return_feats=True, device=DEV)
    assert notes == want_notes and torch.equal(feats, want_feats)


def test_noise_sweep_writes_the_noisy_wavs(tmp_path):
    cfg = PRESETS["tiny-group"]
    hd = Wt.seeded_head_state_dict(cfg.hidden_size, 20, seed=32)
    enc = S.HuggingFaceWav2Vec2("tiny-group", None, config=cfg, precision="fp32", seed=31).to(DEV)
    head = S.Linear(20, input_size=cfg.hidden_size)
    head.load_state_dict(hd)
    head = head.to(DEV)
    tr = S.SongTranscriber(enc, head, sample_rate=16000, dur_threshold=0.25)
    n = 9001
    g = torch.Generator().manual_seed(5)
    clean = (0.2 * torch.randn(n, generator=g)).to(DEV)
    noise = (0.1 * torch.randn(n, generator=g)).to(DEV)
    folder = str(tmp_path / "song")
    got = S.NoiseSweep(tr).run(clean, noise, song_folder=folder, noise_type="white", write_wavs=True)
    assert list(got) == list(S.SNRS_DB) and len(S.SNRS_DB) == 5
    rows = S.mix_at_snrs(clean, noise, S.SNRS_DB)
    for s, snr in enumerate(S.SNRS_DB):
        path = S.noisy_wav_path(folder, "white", snr)
        assert tuple(audio_io.info(path)) == (16000, n, 1, 32, "PCM_F")
        wav, fs = S.load(path, device=DEV)
        assert fs == 16000 and wav.shape == (1, n) and torch.equal(wav[0].view(torch.int32), rows[s].contiguous().view(torch.int32))
    import os
    quiet = str(tmp_path / "quiet")
    S.NoiseSweep(tr, snrs_db=(0,)).run(clean, noise, song_folder=quiet, noise_type="white")      # the default writes no wav
    assert not os.path.exists(S.noisy_wav_path(quiet, "white", 0))
    with pytest.raises(ValueError):
        S.NoiseSweep(tr).run(clean, noise, write_wavs=True)
