"""Resampling and stereo downmix on the GPU: the two steps every recipe's data preparation runs before anything else
(``MIR_ST500/prepare_benchmarks.py:49-72``, its twin under ``N20EMv2/audio_only/``, ``N20EMv2/audio_visual/synthesis_noise.py:18-48``
``resample_wav``): ``Resample(orig_freq=fs, new_freq=16000)`` and, for a stereo file, ``.mean(dim=0, keepdim=True)``.

Which resampler: the recipe scripts call ``torchaudio.transforms.Resample``; this module is pinned to the class the reference vendors,
``speechbrain.processing.speech_augmentation.Resample`` (``speech_augmentation.py:479-789``), which describes itself as a modification of
torchaudio's and is Kaldi's ``LinearResample``: a Hann-windowed sinc of ``lowpass_filter_width`` zero crossings, cut off at
``0.99 * 0.5 * min(orig, new)``.  No bit parity with torchaudio (or librosa) is claimed.

* ``resample_table``: the filter table of that class -- ``first`` (the input offset of each phase's first tap) and ``weights`` -- built on
  the CPU in fp32 torch ops in the reference's order, so the bits are the reference's (``tests/golden/resample.pt``).
* ``Resample``: the reference's constructor and ``forward`` over ``svt_resample`` (``csrc/resample.hip``): ONE launch for all rows
  where the reference loops over the phases (160 at 44.1 -> 16 kHz) with five ops per phase over the whole output.  Each output is one
  fp32 sum of its W products; the reference sums the same products in conv1d's order, so the two agree to rounding, not bit for bit.
* ``resample_to_mono``: both preparation steps in one call (the downmix is fused into the kernel: ``0.5 * (y_left + y_right)``).
* ``SpeedPerturb``: the reference's class over this ``Resample`` (the recipes' commented-out ``augmentation:`` block,
  ``train_audio_ssl.yaml:91-93``); it makes the same ``torch.rand`` / ``torch.randint`` draws in the same order.

Wav files are read and written by ``audio_io`` (``load`` puts the decoded waveform on the GPU, where these classes want it).  Waveforms
must be on the GPU; there is no CPU fallback.
"""
from __future__ import annotations

import math
from typing import Dict, Sequence, Tuple

import torch

from . import _lib


def output_samples(n_in: int, orig_freq: int, new_freq: int) -> int:
    """``Resample._output_samples`` (Kaldi's ``GetNumOutputSamples``; C ABI: ``svt_resample_output_samples``): the outputs whose time lies
    in ``[0, n_in / orig_freq)``, counted exactly in ticks of ``1 / lcm(orig, new)``."""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    g = math.gcd(orig_freq, new_freq)
    per_in, per_out = new_freq // g, orig_freq // g
    interval = int(n_in) * per_in
    if interval <= 0:
        return 0
    last = interval // per_out
    if last * per_out == interval:
        last -= 1
    return last + 1


# include/svt_mi355.h: SVT_RESAMPLE_TILE_OUTPUTS / SVT_RESAMPLE_LDS_BYTES / SVT_RESAMPLE_MAX_WORKGROUPS.  A call with more than
# MAX_WORKGROUPS (row, tile) pairs sends its workgroups on a second trip over the tiles
TILE_OUTPUTS = 1024
LDS_BYTES = 65536
MAX_WORKGROUPS = 768


def units_per_tile(P: int, W: int, S: int, downmix: bool = False) -> int:
    """G of a ``svt_resample`` launch: a workgroup owns G units = G * P consecutive outputs of a row.  The smallest G with
    ``G * P >= TILE_OUTPUTS``, lowered until the table (P rows of ``W | 1`` weights, P first indices, 2 words) and the input span
    (``G * S + 2 * W`` samples, up to a multiple of 4, per channel) fit ``LDS_BYTES``; 0: the table does not fit at all."""
    G = -(-TILE_OUTPUTS // P)
    while G >= 1 and 4 * ((2 if downmix else 1) * ((G * S + 2 * W + 3) // 4 * 4) + P * (W | 1) + P + 2) > LDS_BYTES:
        G -= 1
    return G


def resample_table(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """``(first int32 (P,), weights fp32 (P, W), S)`` of ``Resample._indices_and_weights`` (``speech_augmentation.py:720-789``): with
    ``g = gcd(orig, new)``, ``S = orig / g``, ``P = new / g``, output ``n * P + p`` is ``sum_j x[n * S + first[p] + j] * weights[p][j]``.
    CPU tensors; fp32 torch ops in the reference's order (masked assignments included), so the bits are the reference's."""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq < 1 or new_freq < 1:
        raise ValueError("sampling rates must be positive")
    g = math.gcd(orig_freq, new_freq)
    S, P = orig_freq // g, new_freq // g
    min_freq = min(orig_freq, new_freq)
    cutoff = 0.99 * 0.5 * min_freq
    window = lowpass_filter_width / (2.0 * cutoff)
    t = torch.arange(start=0.0, end=P)
    t /= new_freq
    lo = torch.ceil((t - window) * orig_freq)
    hi = torch.floor((t + window) * orig_freq)
    W = (hi - lo + 1).max()
    j = torch.arange(W)
    delta = ((lo.unsqueeze(1) + j.unsqueeze(0)) / orig_freq) - t.unsqueeze(1)
    w = torch.zeros_like(delta)
    inside = delta.abs().lt(window)
    w[inside] = 0.5 * (1 + torch.cos(2 * math.pi * cutoff / lowpass_filter_width * delta[inside]))   # Hann window
    zero = delta.eq(0.0)
    w[~zero] *= torch.sin(2 * math.pi * cutoff * delta[~zero]) / (math.pi * delta[~zero])             # sinc
    w[zero] *= 2 * cutoff                                                                             # its limit at 0
    w /= orig_freq
    return lo.to(torch.int32), w, S


def _launch(x: torch.Tensor, table, out: torch.Tensor, downmix: bool) -> None:
    """x: (rows, n_in) fp32 contiguous on the GPU; out: (rows or rows / 2, n_out) contiguous."""
    first, weights, S = table
    lib = _lib.load()
    _lib.check(lib.svt_resample(_lib.ptr(x), x.shape[0], x.shape[1], x.shape[1], _lib.ptr(weights), _lib.ptr(first), weights.shape[0],
                                weights.shape[1], S, _lib.ptr(out), out.shape[1], out.shape[1], int(downmix), _lib.dev_index(x.device),
                                _lib.stream_ptr(x.device)), "svt_resample")


class Resample(torch.nn.Module):
    """``speechbrain.processing.speech_augmentation.Resample``: ``[batch, time]`` -> ``[batch, time']``, ``[batch, time, channels]`` ->
    ``[batch, time', channels]``, fp32 out; equal rates return the input object.  The table is built once on the CPU and uploaded once
    per device."""

    def __init__(self, orig_freq: int = 16000, new_freq: int = 16000, lowpass_filter_width: int = 6):
        super().__init__()
        self.orig_freq, self.new_freq, self.lowpass_filter_width = orig_freq, new_freq, lowpass_filter_width
        g = math.gcd(int(orig_freq), int(new_freq))
        self.conv_stride, self.conv_transpose_stride = int(orig_freq) // g, int(new_freq) // g   # S and P, under the reference's names
        self.output_samples = self.conv_transpose_stride
        self._host = None
        self._tables: Dict[torch.device, tuple] = {}

    def table(self, device=None):
        """``(first, weights, S)`` on the CPU, or uploaded to ``device`` (cached)."""
        if self._host is None:
            self._host = resample_table(self.orig_freq, self.new_freq, self.lowpass_filter_width)
        if device is None:
            return self._host
        device = torch.device(device)
        if device not in self._tables:
            first, weights, S = self._host
            self._tables[device] = (first.to(device), weights.contiguous().to(device), S)
        return self._tables[device]

    @property
    def first_indices(self):
        return self.table()[0]

    @property
    def weights(self):
        return self.table()[1]

    def _output_samples(self, input_num_samp: int) -> int:
        return output_samples(input_num_samp, self.orig_freq, self.new_freq)

    def _rows(self, x: torch.Tensor, downmix: bool = False) -> torch.Tensor:
        """(rows, n_in) -> (rows, n_out), or (rows / 2, n_out) with the channel pairs averaged."""
        if not x.is_cuda:
            raise _lib.SvtError("resampling needs its waveforms on the GPU; there is no CPU fallback")
        x = x.detach().to(torch.float32).contiguous()
        rows, n_in = x.shape
        out = torch.empty((rows // 2 if downmix else rows, self._output_samples(n_in)), dtype=torch.float32, device=x.device)
        if out.numel():
            _launch(x, self.table(x.device), out, downmix)
        return out

    @torch.no_grad()
    def forward(self, waveforms: torch.Tensor) -> torch.Tensor:
        if self.orig_freq == self.new_freq:
            return waveforms
        if waveforms.dim() == 2:
            return self._rows(waveforms)
        if waveforms.dim() == 3:
            b, _, c = waveforms.shape
            y = self._rows(waveforms.transpose(1, 2).reshape(b * c, -1))
            return y.view(b, c, -1).transpose(1, 2)
        raise ValueError("Input must be 2 or 3 dimensions")


_resamplers: Dict[tuple, Resample] = {}


def resample_to_mono(wave: torch.Tensor, orig_freq: int, new_freq: int = 16000) -> torch.Tensor:
    """The preparation scripts' two steps in one call: ``wave`` is ``(n,)`` or ``(C, n)`` with C = 1 or 2 at ``orig_freq`` on the GPU;
    returns the mono ``(n',)`` fp32 track at ``new_freq``.  Stereo is resampled and averaged in one launch, ``0.5 * (y_0 + y_1)`` -- what
    ``Resample`` followed by ``.mean(dim=0)`` gives.  Equal rates: the track itself (mono) or the plain mean (stereo)."""
    if not torch.is_tensor(wave):
        raise TypeError("wave must be a tensor")
    if wave.dim() == 1:
        wave = wave.unsqueeze(0)
    if wave.dim() != 2 or wave.shape[0] not in (1, 2):
        raise ValueError(f"expected a waveform of shape (n,), (1, n) or (2, n), got {tuple(wave.shape)}")
    if int(orig_freq) == int(new_freq):
        return wave[0] if wave.shape[0] == 1 else wave.to(torch.float32).mean(dim=0)
    key = (int(orig_freq), int(new_freq))
    if key not in _resamplers:
        _resamplers[key] = Resample(*key)
    return _resamplers[key]._rows(wave, downmix=wave.shape[0] == 2)[0]


class SpeedPerturb(torch.nn.Module):
    """``speechbrain.processing.speech_augmentation.SpeedPerturb`` (``speech_augmentation.py:403-476``): resample to
    ``orig_freq * speed // 100`` for a randomly drawn ``speed`` and keep calling it ``orig_freq``.  The draws are the reference's, in its
    order -- ``torch.rand(1)`` against ``perturb_prob``, then ``torch.randint(len(speeds), (1,))`` -- so a seeded run picks the same speeds."""

    def __init__(self, orig_freq: int, speeds: Sequence[int] = (90, 100, 110), perturb_prob: float = 1.0):
        super().__init__()
        self.orig_freq, self.speeds, self.perturb_prob = orig_freq, list(speeds), perturb_prob
        self.samp_index = 0
        self.resamplers = [Resample(orig_freq=orig_freq, new_freq=orig_freq * speed // 100) for speed in self.speeds]

    @torch.no_grad()
    def forward(self, waveform: torch.Tensor) -> torch.Tensor:
        if torch.rand(1) > self.perturb_prob:
            return waveform.clone()
        self.samp_index = torch.randint(len(self.speeds), (1,))[0]
        return self.resamplers[self.samp_index](waveform)
