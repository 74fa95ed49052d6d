"""svt_noise_mix on the GPU (csrc/noise_mix.hip): every element of every row against the fp64 formula under the limit of
tests/noise_limit.py (a bound derived from the roundings, held by a correct fp32 evaluation and missed by the mutants of
tests/test_noise_limit.py), the amplitudes against exactly rounded fp64 means, unaligned tracks and padded rows with poisoned gaps, the
argument checks, bitwise reproducibility, the reference's own mixtures recorded in tests/golden/noise_mix.pt, and the sweep driver.

Sizes: 1, 3, 4, 5 (below, at and just past one 16-byte piece), 1027 (one workgroup, head and tail peels), 300 001 (several workgroups of
both kernels; a second trip of the sums' loop, whose grid holds AMP_WORKGROUPS x 1024 samples) and SECOND_TRIP: the smallest length at
which the mix kernel's capped grid (MIX_MAX_WORKGROUPS workgroups x 256 threads x 4 samples) takes a second trip of its loop."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import noise_limit as NL  # noqa: E402
import svt_speechbrain_amd as S  # noqa: E402
from oracle import svt_oracle as O  # noqa: E402
from svt_speechbrain_amd import _lib, noise as N, weights as W  # noqa: E402
from svt_speechbrain_amd.config import PRESETS  # noqa: E402

DEV = "cuda:0"
SECOND_TRIP = N.MIX_MAX_WORKGROUPS * N.SAMPLES_PER_WORKGROUP + 4   # 16-byte-aligned rows: one 16-byte piece is left for the second trip
SIZES = (1, 3, 4, 5, 1027, 300001, SECOND_TRIP)
POISON = 0x7FC0DEAD   # a NaN with a payload: a write of any value, NaN included, changes the bits
GUARD = 64
INVALID, WORKSPACE = -1, -4


def mix(a, v, snrs=NL.SNRS_DB, off=(0, 0, 0), pad=0, amps=True, ws_bytes=None, n=None, expect=0):
    """One svt_noise_mix call through the C ABI on copies of a, v placed off[0] / off[1] floats behind a fresh allocation, rows of n + pad
    floats starting off[2] floats (+ GUARD) behind another.  Returns (rows (S, n), amplitudes (2,) fp64 or None, the whole output buffer as
    int32, a mask of the elements the call may write)."""
    lib = _lib.load()
    n = a.shape[0] if n is None else n
    S_, ld = len(snrs), max(n, 1) + pad
    bufs = []
    for t, o in ((a, off[0]), (v, off[1])):
        b = torch.zeros(o + max(t.shape[0], 1), dtype=torch.float32, device=DEV)
        b[o:o + t.shape[0]] = t.to(DEV)
        bufs.append(b[o:])
    out = torch.full((GUARD + off[2] + S_ * ld + GUARD,), POISON, dtype=torch.int32, device=DEV)
    first = GUARD + off[2]
    amp = torch.full((2,), float("nan"), dtype=torch.float64, device=DEV) if amps else None
    need = 2 * N.AMP_WORKGROUPS * 8
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc = lib.svt_noise_mix(_lib.ptr(bufs[0]), _lib.ptr(bufs[1]), n, (C.c_float * S_)(*snrs), S_, _lib.ptr(out) + 4 * first, ld,
                           _lib.ptr(amp) if amps else None, _lib.ptr(ws), need if ws_bytes is None else ws_bytes, 0, _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == expect, (rc, _lib.last_error())
    may = torch.zeros(out.shape, dtype=torch.bool, device=DEV)
    may[first:first + S_ * ld].view(S_, ld)[:, :n] = True
    rows = out[first:first + S_ * ld].view(S_, ld)[:, :n].view(torch.float32)
    return rows, amp, out, may


def untouched(out, may):
    return bool((out[~may] == POISON).all())


_cache = {}


def case(n):
    """(a, v, fp64 formula, limit, exact amplitudes) of a size, computed once and never changed."""
    if n not in _cache:
        a, v = NL.seeded_track(n, 100 + n % 89), NL.seeded_track(n, 200 + n % 97, "noise")
        amps = (NL.mean_abs_exact(a), NL.mean_abs_exact(v))
        ref, M = NL.formula(a, v, NL.SNRS_DB, amps)
        _cache[n] = (a, v, ref, NL.limit(M), amps)
    return _cache[n]


def check_amps(amp, want):
    for got, w in zip(amp.cpu().tolist(), want):
        assert abs(got - w) <= 2.0 ** -50 * w, (got, w, abs(got - w) / w * 2.0 ** 53)


@pytest.mark.parametrize("n", SIZES)
def test_every_element_inside_the_limit(n):
    a, v, ref, lim, amps = case(n)
    rows, amp, out, may = mix(a, v)
    r = NL.worst(rows.cpu(), ref, lim)
    print(f"n = {n}: worst error {r:.3f} of the limit; amplitudes {amp.cpu().tolist()}")
    assert r <= 1.0, (n, r)
    check_amps(amp, amps)
    assert untouched(out, may)


@pytest.mark.parametrize("n", (5, 1027, 300001))
@pytest.mark.parametrize("off", ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (3, 2, 1)))
def test_unaligned_tracks_and_padded_rows(n, off):
    """clean, noise and out each one float off a fresh allocation, alone and together; rows n + 5 apart: the gaps between the rows and the
    guards around them come back bit for bit."""
    a, v, ref, lim, amps = case(n)
    rows, amp, out, may = mix(a, v, off=off, pad=5)
    assert (_lib.ptr(out) + 4 * (GUARD + off[2])) % 16 == 4 * off[2] % 16
    assert NL.worst(rows.cpu(), ref, lim) <= 1.0
    check_amps(amp, amps)
    assert untouched(out, may)


def test_python_entry_points():
    a, v, ref, lim, amps = case(1027)
    got, amp = S.mix_at_snrs(a.to(DEV), v.to(DEV)[None], return_amplitudes=True)
    assert got.shape == (5, 1027) and got.dtype == torch.float32 and got.is_cuda and NL.worst(got.cpu(), ref, lim) <= 1.0
    check_amps(amp, amps)
    wide = torch.zeros(5, 1040, device=DEV)
    assert S.mix_at_snrs(a.to(DEV), v.to(DEV), out=wide[:, 3:1030]) .data_ptr() == wide[:, 3:].data_ptr()
    assert torch.equal(wide[:, 3:1030], got) and wide[:, :3].abs().max() == 0 and wide[:, 1030:].abs().max() == 0
    amp1 = S.compute_amplitude(a.to(DEV))
    assert amp1.dim() == 0 and amp1.is_cuda and amp1.dtype == torch.float32 and amp1.item() == torch.tensor(amps[0]).float().item()
    with pytest.raises(ValueError):
        S.mix_at_snrs(a.to(DEV), v.to(DEV), snrs_db=range(9))
    with pytest.raises(ValueError):
        S.mix_at_snrs(a.to(DEV), v.to(DEV), out=torch.zeros(5, 1027, device=DEV).t().contiguous().t())


def test_one_and_eight_rows():
    a, v, _, _, amps = case(1027)
    for snrs in ((5,), (-10, -5, 0, 5, 10, 15, 20, 25)):
        ref, M = NL.formula(a, v, snrs, amps)
        rows, amp, out, may = mix(a, v, snrs=snrs, pad=2)
        assert rows.shape[0] == len(snrs) and NL.worst(rows.cpu(), ref, NL.limit(M)) <= 1.0
        check_amps(amp, amps)
        assert untouched(out, may)


def test_refusals_write_nothing():
    a, v = case(1027)[:2]
    for kw, rc in ((dict(snrs=tuple(range(9))), INVALID), (dict(n=0), INVALID), (dict(ws_bytes=2 * N.AMP_WORKGROUPS * 8 - 1), WORKSPACE),
                   (dict(snrs=(float("nan"),)), INVALID), (dict(pad=-1), INVALID)):
        rows, amp, out, may = mix(a, v, expect=rc, **kw)
        assert bool((out == POISON).all()) and bool(torch.isnan(amp).all()), kw
        assert _lib.last_error().startswith("svt_noise_mix")
    assert _lib.load().svt_noise_mix_workspace_bytes(1027, 5) == 2 * N.AMP_WORKGROUPS * 8


def test_silent_tracks():
    a, v = case(300001)[:2]
    z = torch.zeros_like(a)
    rows, amp, _, _ = mix(a, z)                         # A_v = 0: c2 = 0, the rows are c1 * a
    assert bool(torch.isfinite(rows).all()) and amp.cpu().tolist()[1] == 0.0
    ref = torch.stack([(1 - NL.factor(s)) * a.double() for s in NL.SNRS_DB])
    assert NL.worst(rows.cpu(), ref, NL.limit(ref.abs())) <= 1.0
    rows, amp, _, _ = mix(z, v)                         # a silent song stays silent
    assert bool((rows == 0).all()) and amp.cpu().tolist()[0] == 0.0
    rows, _, _, _ = mix(z, z)
    assert bool((rows == 0).all())


@pytest.mark.parametrize("n", (300001, SECOND_TRIP))
def test_two_calls_give_the_same_bits(n):
    a, v = case(n)[:2]
    r1, a1, _, _ = mix(a, v, off=(1, 0, 1), pad=3)
    r2, a2, _, _ = mix(a, v, off=(1, 0, 1), pad=3)
    assert torch.equal(r1.view(torch.int32), r2.view(torch.int32)) and torch.equal(a1.view(torch.int64), a2.view(torch.int64))


def test_fixture_samples_of_the_reference():
    """Every (song, type, SNR) of tests/golden/noise_mix.pt: the kernel's mixture at the recorded samples is within (1 + ref_vs_fp64) limit of
    what the reference's synthesis_noise.py saved -- its own distance from the formula, read from the fixture, added by the triangle
    inequality."""
    fx = NL.load_fixture()
    songs, tracks = NL.fixture_inputs(fx)["songs"], NL.fixture_noise_tracks(fx)
    assert len(fx["mix"]) == 2 * 4 * 5
    for (song, typ), v in tracks.items():
        a = songs[song]
        idx = torch.arange(0, a.shape[0], NL.STEP)
        got = S.mix_at_snrs(a.to(DEV), v.to(DEV)).cpu()[:, idx]
        _, M = NL.formula(a[idx], v[idx], NL.SNRS_DB, (NL.mean_abs_exact(a), NL.mean_abs_exact(v)))
        for s, snr in enumerate(NL.SNRS_DB):
            rec = fx["mix"][song, typ, snr]
            r = NL.worst(got[s], rec["samples"].double(), (1 + rec["ref_vs_fp64"]) * NL.limit(M[s]))
            assert r <= 1.0, (song, typ, snr, r, rec["ref_vs_fp64"])


def test_noise_sweep(tmp_path):
    """3.4 utterances of 0.25 s at two SNRs: run() returns what transcribe() gives for each row on its own, writes the features where the
    audio-visual recipe reads them, and both agree with the CPU oracle on the fp64 formula's mixture (rounded to fp32) within the bound of
    test_gpu_parity.py::test_song_transcriber_matches_oracle_per_utterance for this preset in fp32: equal notes, features within 1e-3."""
    cfg = PRESETS["tiny-group"]
    sd = W.seeded_encoder_state_dict(cfg, seed=31)
    hd = W.seeded_head_state_dict(cfg.hidden_size, 20, seed=32)
    enc = S.HuggingFaceWav2Vec2("tiny-group", None, config=cfg, precision="fp32", seed=31).to(DEV)
    head = S.Linear(20, input_size=cfg.hidden_size)
    head.load_state_dict(hd)
    head = head.to(DEV)
    n, snrs = int(3.4 * 4000), (-10, 10)
    clean, noise = NL.seeded_track(n, 77), NL.seeded_track(n, 78, "noise")
    tr = S.SongTranscriber(enc, head, sample_rate=16000, dur_threshold=0.25)
    bounds = S.utterance_bounds(n, 16000, 0.25)
    assert len(bounds) == 3 and bounds[-1] == (8000, n)
    folder = str(tmp_path / "song")
    got = S.NoiseSweep(tr, snrs_db=snrs).run(clean.to(DEV), noise.to(DEV), song_folder=folder, noise_type="white")
    assert list(got) == list(snrs)
    rows = S.mix_at_snrs(clean.to(DEV), noise.to(DEV), snrs)
    ref_mix = NL.formula(clean, noise, snrs)[0].float()
    for s, snr in enumerate(snrs):
        notes, feats = got[snr]
        alone_notes, alone_feats = tr.transcribe(rows[s], return_feats=True)
        assert notes == alone_notes and torch.equal(feats, alone_feats)
        path = S.feature_path(folder, True, "white", snr)
        assert path.endswith(f"noise_data/white/SNR_{snr}dB_feats.pt") and torch.equal(torch.load(path), feats.cpu())
        info, ref_feats = [], []
        with torch.no_grad():
            for lo, hi in bounds:
                f = O.encoder_forward(sd, cfg, ref_mix[s, lo:hi][None])
                p_on, p_off, octv, pc = O.decode_frames(O.head_forward(f, hd["w.weight"], hd["w.bias"]))
                info += list(zip(p_on[0].numpy(), p_off[0].numpy(), octv[0].tolist(), pc[0].tolist()))
                ref_feats.append(f[0])
        ref_feats = torch.cat(ref_feats)
        err = (feats.cpu() - ref_feats).abs().max().item()
        print(f"SNR {snr} dB: {len(notes)} notes, features max|err| vs oracle {err:.3e}")
        assert notes == O.frame2note(info, 0.4, 0.5)
        assert feats.shape == ref_feats.shape and err < 1e-3
