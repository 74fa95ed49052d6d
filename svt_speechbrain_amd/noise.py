"""Noisy copies of a song at the recipes' five SNRs (``N20EMv2/audio_visual/synthesis_noise.py``), the input of config C4 as its yaml
ships it (``train_rca_av.yaml:11-13``: ``noise_type: natural``, ``snr_db: -10``, ``add_noise: True``).

* ``mix_at_snrs``: the arithmetic of ``synthesis_noise.py:123-137`` (identical in ``synthesis_accomp`` / ``_white`` / ``_babble`` /
  ``_natural``) on the GPU, all SNRs in one call (``svt_noise_mix``: two launches, nine passes over a track instead of about sixty).
  With ``f = 1 / (10 ** (snr / 20) + 1)`` (Python double), ``A_a = mean|clean|``, ``A_v = mean|noise|``::

      out[s] = (1 - f_s) * clean + (f_s * A_a / (A_v + 1e-14)) * noise

  The reference rescales its noise tensor IN PLACE, so SNR k starts from the track already rescaled for SNR k-1 and takes its amplitude
  again: the same formula with the original track in exact arithmetic, a few ulps of drift per step in fp32.  This module always starts
  from the original track.
* ``compute_amplitude``: the default branch of ``speechbrain.processing.signal_processing.compute_amplitude`` (``mean(|x|)`` of the track).
* the host-side assembly of the babble and natural tracks (``assemble_noise_track``, ``split_natural_files`` and the duration filters):
  copies and zero padding over CPU tensors, once per song; seeded and called like the reference (``random.seed(1234)``, ``:478-482``) they
  make the same picks.

Reading, resampling and writing audio files stay with the caller; white noise is the caller's ``torch.randn_like`` track.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import OrderedDict
from typing import Dict, Iterable, Mapping, Sequence, Union

import torch

from . import _lib

SNRS_DB = (-10, -5, 0, 5, 10)   # synthesis_noise.py:123 (and :166, :292, :454)
NOISE_TYPES = ("accomp", "white", "babble", "natural")
MAX_SNRS = 8                    # rows of one svt_noise_mix call
# include/svt_mi355.h: SVT_NOISE_AMP_WORKGROUPS / SVT_NOISE_MIX_MAX_WORKGROUPS, workgroups of 256 threads x 4 samples.  A track longer than
# MIX_MAX_WORKGROUPS * SAMPLES_PER_WORKGROUP (+ the head peel of up to 3) takes a second trip of the mix kernel's grid-stride loop.
AMP_WORKGROUPS = 256
MIX_MAX_WORKGROUPS = 2048
SAMPLES_PER_WORKGROUP = 1024


def _tracks(clean: torch.Tensor, noise: torch.Tensor):
    """1-D views of the two tracks (the reference's ``(1, n)`` is accepted): equal lengths (``synthesis_noise.py:121, 286, 449``), on the GPU."""
    if not (torch.is_tensor(clean) and torch.is_tensor(noise)):
        raise TypeError("clean and noise must be tensors")
    tracks = []
    for name, t in (("clean", clean), ("noise", noise)):
        if t.dim() == 2 and t.shape[0] == 1:
            t = t[0]
        if t.dim() != 1:
            raise ValueError(f"{name}: expected a mono track of shape (n,) or (1, n), got {tuple(t.shape)}")
        tracks.append(t)
    a, v = tracks
    if a.shape[0] != v.shape[0]:
        raise ValueError(f"clean and noise must have the same length, got {a.shape[0]} and {v.shape[0]} samples")
    if a.shape[0] < 1:
        raise ValueError("empty track")
    if not (a.is_cuda and v.is_cuda):
        raise _lib.SvtError("noise mixing needs its tracks on the GPU; there is no CPU fallback")
    if a.device != v.device:
        raise ValueError("clean and noise live on different devices")
    return a.detach().to(torch.float32).contiguous(), v.detach().to(torch.float32).contiguous()


def _call(a, v, snrs, out_ptr, ld, amps):
    lib = _lib.load()
    n, S = a.shape[0], len(snrs)
    need = lib.svt_noise_mix_workspace_bytes(n, S)
    if need < 0:
        raise ValueError(f"svt_noise_mix: {S} SNRs (1..{MAX_SNRS}) over {n} samples")
    ws = torch.empty(int(need), dtype=torch.uint8, device=a.device)   # per call: calls on different streams share nothing
    snr_c = (C.c_float * S)(*[float(s) for s in snrs])
    _lib.check(lib.svt_noise_mix(_lib.ptr(a), _lib.ptr(v), n, snr_c, S, out_ptr, ld, _lib.ptr(amps) if amps is not None else None,
                                 _lib.ptr(ws), ws.numel(), _lib.dev_index(a.device), _lib.stream_ptr(a.device)), "svt_noise_mix")


def mix_at_snrs(clean: torch.Tensor, noise: torch.Tensor, snrs_db: Sequence[float] = SNRS_DB, out: torch.Tensor = None,
                return_amplitudes: bool = False):
    """``(S, n)`` fp32 mixtures of a clean and a noise track (GPU, equal lengths) at ``snrs_db``, row ``s`` at ``snrs_db[s]``.

    ``out``: an ``(S, n)`` fp32 tensor on the same device with unit stride along time and a row stride >= n (a view of a wider buffer
    will do: nothing is written between the rows); returned as is.  ``return_amplitudes``: also the fp64 pair ``(mean|clean|,
    mean|noise|)`` as a 2-element GPU tensor.  Nothing synchronises.  A silent noise track gives ``(1 - f) * clean``."""
    a, v = _tracks(clean, noise)
    snrs = list(snrs_db)
    n, S = a.shape[0], len(snrs)
    if not 1 <= S <= MAX_SNRS:
        raise ValueError(f"between 1 and {MAX_SNRS} SNRs per call, got {S}")
    if out is None:
        out = torch.empty((S, n), dtype=torch.float32, device=a.device)
    elif (out.dtype != torch.float32 or out.device != a.device or tuple(out.shape) != (S, n) or (n > 1 and out.stride(1) != 1)
          or (S > 1 and out.stride(0) < n)):
        raise ValueError(f"out must be a ({S}, {n}) float32 tensor on {a.device} with unit stride along time and a row stride >= {n}")
    amps = torch.empty(2, dtype=torch.float64, device=a.device) if return_amplitudes else None
    _call(a, v, snrs, _lib.ptr(out), out.stride(0) if S > 1 else n, amps)
    return (out, amps) if return_amplitudes else out


def compute_amplitude(waveforms: torch.Tensor, lengths=None, amp_type: str = "avg", scale: str = "linear") -> torch.Tensor:
    """``mean(|x|)`` of one GPU track as a 0-dim tensor of its dtype: the default branch of the reference function
    (``speechbrain/processing/signal_processing.py:15-66``), summed in fp64 in a fixed order."""
    if lengths is not None or amp_type != "avg" or scale != "linear":
        raise NotImplementedError("only the default branch is built: amp_type='avg', scale='linear', no lengths")
    x, _ = _tracks(waveforms, waveforms)
    amps = torch.empty(2, dtype=torch.float64, device=x.device)
    _call(x, x, [0.0], None, x.shape[0], amps)   # no output rows: the sums alone
    return amps[0].to(waveforms.dtype if waveforms.dtype.is_floating_point else torch.float32)


# ---- host-side assembly of the babble / natural tracks: CPU tensors, once per song ----

def natural_keep(n_samples: int, sample_rate: int = 16000) -> bool:
    """The natural pool's filter: files of 1 to 10 seconds, both ends included (``synthesis_noise.py:331, 343``)."""
    return 1 <= n_samples / sample_rate <= 10


def babble_keep(n_samples: int, sample_rate: int = 16000) -> bool:
    """The babble pool's filter: files of exactly 10 seconds (``synthesis_noise.py:200``)."""
    return n_samples / sample_rate == 10


def babble_split(path: str) -> str:
    """A babble file's split is its file name up to the first ``-`` (``synthesis_noise.py:198``)."""
    return path.split("/")[-1].split("-")[0]


def split_natural_files(keys_free_sound: Iterable[str], keys_sound_bible: Iterable[str], rng) -> "OrderedDict[str, str]":
    """``{key: "train" | "valid" | "test"}`` of the kept natural files as ``synthesis_noise.py:345-368`` assigns them: each folder's keys
    are shuffled on their own (two ``rng.shuffle`` calls, free-sound first) and a running index ``i`` over the shuffled list decides:
    ``i <= len * 3 / 4`` train, ``len * 3 / 4 < i <= len * 7 / 8`` valid, else test (``<=``: train gets one more than three quarters).
    The result keeps the reference's pool order -- the keys as given, free-sound before sound-bible -- which is the order
    ``rng.choice`` later indexes."""
    out: "OrderedDict[str, str]" = OrderedDict()
    folders = [list(keys_free_sound), list(keys_sound_bible)]
    shuffled = [list(k) for k in folders]
    for s in shuffled:
        rng.shuffle(s)
    assigned: Dict[str, str] = {}
    for s in shuffled:
        for i, key in enumerate(s):
            assigned[key] = "train" if i <= len(s) * 3 / 4 else "valid" if i <= len(s) * 7 / 8 else "test"
    for keys in folders:
        for key in keys:
            out[key] = assigned[key]
    return out


def noise_pools(files: Mapping[str, torch.Tensor], splits: Mapping[str, str]) -> Dict[str, "OrderedDict[str, torch.Tensor]"]:
    """``{"train": {key: track}, "valid": ..., "test": ...}`` in the order of ``splits`` (``synthesis_noise.py:213-226, 374-387``)."""
    pools = {k: OrderedDict() for k in ("train", "valid", "test")}
    for key, split in splits.items():
        if split in pools:
            pools[split][key] = files[key]
    return pools


def natural_pools(free_sound: Mapping[str, torch.Tensor], sound_bible: Mapping[str, torch.Tensor], rng, sample_rate: int = 16000):
    """The three natural pools from the two folders' ``{key: track}`` (in the order the files are listed): duration filter, split,
    pools.  Returns ``(pools, splits)``."""
    kept = [OrderedDict((k, t) for k, t in folder.items() if natural_keep(t.shape[-1], sample_rate)) for folder in (free_sound, sound_bible)]
    splits = split_natural_files(kept[0].keys(), kept[1].keys(), rng)
    files = dict(kept[0])
    files.update(kept[1])
    return noise_pools(files, splits), splits


def babble_pools(files: Mapping[str, torch.Tensor], sample_rate: int = 16000):
    """The three babble pools from ``{path: track}`` (in the order the files are listed): only files of exactly 10 s, keyed by file
    name, split by the name's prefix (``synthesis_noise.py:195-226``).  Returns ``(pools, splits)``."""
    kept, splits = OrderedDict(), OrderedDict()
    for path, t in files.items():
        if babble_keep(t.shape[-1], sample_rate):
            name = path.split("/")[-1]
            kept[name] = t
            splits[name] = babble_split(path)
    return noise_pools(kept, splits), splits


def assemble_noise_track(pool: Union[Mapping[str, torch.Tensor], Sequence[torch.Tensor]], n_samples: int, rng, sample_rate: int = 16000,
                         duration_thrd: float = 10, return_picks: bool = False):
    """The noise track of one song, ``n_samples`` long, from the files of ``pool`` (``synthesis_noise.py:243-283`` / ``:406-446``):
    ``round(ceil(n / sample_rate / duration_thrd))`` chunks, one ``rng.choice(list(pool))`` each; a full chunk is its file centred in
    ``duration_thrd`` seconds of zeros (``pad1 = (chunk - len) // 2`` in front, the rest behind); in the last chunk a file no longer than
    the remainder is centred in the remainder and a longer one is cut to its first ``remainder`` samples.  ``pool``: the tracks (``(len,)``
    or ``(1, len)`` CPU tensors) of the song's split, or a mapping whose values they are, in the reference's pool order; ``rng``: a
    ``random.Random``.  Returns the ``(n_samples,)`` track (and the picked pool indices with ``return_picks``).

    Which pool: ``synthesis_natural`` takes the song's split from its annotation.  ``synthesis_babble`` never does -- it reuses the
    variable its file loop left behind (``:198``, ``:250-255``), so every song draws from the pool of the LAST FILE LISTED.  That is not
    reproduced here: the caller passes the pool it means."""
    files = [t.reshape(-1) for t in (pool.values() if isinstance(pool, Mapping) else pool)]
    if n_samples < 1 or not files:
        raise ValueError("assemble_noise_track: an empty song or an empty pool")
    chunk = round(sample_rate * duration_thrd)
    length = round(math.ceil(n_samples / sample_rate / duration_thrd))
    rem = n_samples - (length - 1) * chunk
    pieces, picks = [], []
    for utter in range(length):
        data = rng.choice(files)
        picks.append(next(i for i, t in enumerate(files) if t is data))
        room = chunk if utter < length - 1 else rem
        if data.shape[0] <= room:
            pad1 = (room - data.shape[0]) // 2
            pieces += [torch.zeros(pad1, dtype=data.dtype), data, torch.zeros(room - data.shape[0] - pad1, dtype=data.dtype)]
        elif utter < length - 1:
            raise ValueError(f"a pool file of {data.shape[0]} samples is longer than a chunk of {chunk}")
        else:
            pieces.append(data[:room])
    track = torch.cat(pieces)
    assert track.shape[0] == n_samples
    return (track, picks) if return_picks else track
