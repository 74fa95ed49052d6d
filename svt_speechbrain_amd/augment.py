"""Time-domain SpecAugment on the GPU: the optional ``augmentation: !new:speechbrain.lobes.augment.TimeDomainSpecAugment`` block of the
five training yamls (``MIR_ST500/hparams/train_audio_ssl.yaml:91-93``; ``speechbrain/lobes/augment.py:203-298``), which runs
``SpeedPerturb``, ``DropFreq`` and ``DropChunk`` in a row (``speechbrain/processing/speech_augmentation.py:403-476, 876-1140``).

* ``notch_filter`` / ``drop_filter``: the band-reject filter of ``DropFreq`` -- ``signal_processing.py:372-427`` composed as
  ``speech_augmentation.py:958-971`` composes it -- built on the host in fp32 torch ops in the reference's order.
* ``DropFreq``, ``DropChunk``: the reference's constructors and ``forward`` over ``svt_drop_freq_chunk`` (``csrc/drop_freq_chunk.hip``):
  ONE launch for the whole batch where the reference runs a ``conv1d`` between a transpose, a clone and a squeeze, and then a Python loop
  over the batch with one slice assignment per chunk (and, with lengths on the device, two host synchronisations per clip).
* ``TimeDomainSpecAugment``: the lobe.  ``SpeedPerturb`` (``resample.py``) and then ONE ``svt_drop_freq_chunk`` launch that filters and
  drops at once.

Every random draw is the reference's, from the CPU default generator, in its order and with its shapes (``draw_frequencies``,
``draw_chunks``: plain functions that need no GPU), so a run seeded alike drops the same frequencies and the same spans and leaves the
generator in the same state.  The filtered values agree with the reference's ``conv1d`` to rounding (each output here is one fp32 chain of
fused multiply-adds in ascending tap order), the dropped spans exactly.

Speeds other than 100 change the number of samples, and with it the number of frames against frame-level targets; ``speeds=[100]`` is
the length-preserving setting.  Waveforms must be on the GPU; there is no CPU fallback.  Left out: ``noise_factor != 0`` and more than one
channel.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from .resample import SpeedPerturb

FILTER_LENGTH = 101     # DropFreq's filter_length
# include/svt_mi355.h: SVT_DROP_MAX_TAPS / SVT_DROP_TILE_OUTPUTS / SVT_DROP_MAX_WORKGROUPS
MAX_TAPS = 255
TILE_OUTPUTS = 1024
MAX_WORKGROUPS = 8192


def _sinc(x: torch.Tensor, pad: int) -> torch.Tensor:
    """sin(x) / x with the 1 at the middle index put in by hand."""
    return torch.cat([torch.sin(x[:pad]) / x[:pad], torch.ones(1), torch.sin(x[pad + 1:]) / x[pad + 1:]])


def notch_filter(notch_freq, filter_width: int = 101, notch_width: float = 0.05) -> torch.Tensor:
    """``speechbrain.processing.signal_processing.notch_filter``: a low-pass at ``notch_freq`` plus a high-pass at ``notch_freq + 2 *
    notch_width`` (fractions of half the sampling rate), each a sinc under the PERIODIC Blackman window ``torch.blackman_window`` gives,
    normalised by its sum; ``(1, filter_width, 1)`` fp32 on the CPU.  ``notch_freq``: a float or a 0-dim tensor (what ``DropFreq`` passes:
    then ``notch_freq + notch_width`` is an fp32 sum).  The sum is taken out of place and once -- the reference adds in place, into the
    caller's tensor of drawn frequencies; the value is the same."""
    assert 0 < notch_freq <= 1
    assert filter_width % 2 != 0
    pad = filter_width // 2
    inputs = torch.arange(filter_width) - pad
    notch_freq = notch_freq + notch_width

    hlpf = _sinc(3 * (notch_freq - notch_width) * inputs, pad)
    hlpf *= torch.blackman_window(filter_width)
    hlpf /= torch.sum(hlpf)

    hhpf = _sinc(3 * (notch_freq + notch_width) * inputs, pad)
    hhpf *= torch.blackman_window(filter_width)
    hhpf /= -torch.sum(hhpf)
    hhpf[pad] += 1

    return (hlpf + hhpf).view(1, -1, 1)


def drop_filter(frequencies, drop_width: float = 0.05) -> torch.Tensor:
    """The compound filter of ``DropFreq`` for the drawn ``frequencies`` (a 1-d fp32 tensor or a sequence): a delta at the centre tap,
    cross-correlated (``conv1d`` with 50 zeros either side, as ``convolve1d`` runs it) with one ``notch_filter`` after the other.
    ``(101,)`` fp32 on the CPU.  Not symmetric: the periodic window is not, so the taps must not be flipped."""
    frequencies = torch.as_tensor(frequencies, dtype=torch.float32).reshape(-1)
    pad = FILTER_LENGTH // 2
    f = torch.zeros(1, 1, FILTER_LENGTH)
    f[0, 0, pad] = 1
    with torch.no_grad():
        for frequency in frequencies:
            kernel = notch_filter(frequency, FILTER_LENGTH, drop_width)
            f = torch.nn.functional.conv1d(input=f, weight=kernel.transpose(2, 1), stride=1, groups=1, padding=pad)
    return f.reshape(-1).contiguous()


def draw_frequencies(drop_freq_low, drop_freq_high, drop_count_low, drop_count_high, drop_prob) -> Optional[torch.Tensor]:
    """The draws of ``DropFreq.forward``: ``rand(1)`` against ``drop_prob`` (a miss: None, and nothing else is drawn), ``randint(low,
    high + 1, (1,))`` for the count, ``rand(count)`` scaled into ``[low, high)``.  A count of zero gives an empty tensor."""
    if torch.rand(1) > drop_prob:
        return None
    drop_count = torch.randint(low=drop_count_low, high=drop_count_high + 1, size=(1,))
    return torch.rand(drop_count) * (drop_freq_high - drop_freq_low) + drop_freq_low


def draw_chunks(lengths: torch.Tensor, drop_length_low, drop_length_high, drop_count_low, drop_count_high, drop_start, drop_end,
                drop_prob) -> Optional[List[List[Tuple[int, int]]]]:
    """The draws of ``DropChunk.forward`` for clips of ``lengths`` samples (int64, on the CPU): ``rand(1)`` against ``drop_prob`` (a
    miss: None), ``randint(low, high + 1, (B,))`` for the counts, then per clip with a non-zero count ``randint`` for the lengths and
    ``randint(start_min, start_max + 1)`` for the starts, with ``start_max = max(0, start_max - length.max())`` and negative
    ``drop_start`` / ``drop_end`` offset by the clip's length.  Returns the ``(start, end)`` pairs of every clip as drawn (``end`` may lie
    behind the row, as in the reference's slice)."""
    if torch.rand(1) > drop_prob:
        return None
    batch = lengths.shape[0]
    drop_times = torch.randint(low=drop_count_low, high=drop_count_high + 1, size=(batch,))
    pairs: List[List[Tuple[int, int]]] = []
    for i in range(batch):
        count = int(drop_times[i])
        if count == 0:
            pairs.append([])
            continue
        length = torch.randint(low=drop_length_low, high=drop_length_high + 1, size=(count,))
        clip = int(lengths[i])
        start_min = drop_start
        if start_min < 0:
            start_min += clip
        start_max = drop_end
        if start_max is None:
            start_max = clip
        if start_max < 0:
            start_max += clip
        start_max = max(0, start_max - int(length.max()))
        start = torch.randint(low=start_min, high=start_max + 1, size=(count,))
        end = start + length
        pairs.append(list(zip(start.tolist(), end.tolist())))
    return pairs


def sample_lengths(lengths: torch.Tensor, time: int) -> torch.Tensor:
    """``(lengths * time).long()`` as the reference forms it -- one fp32 product per clip, truncated -- on the CPU.  ``lengths`` on the
    GPU costs one device-to-host copy of its B values (the product of two fp32 numbers is the same number on either side)."""
    return (lengths.detach().cpu() * time).long()


def slice_pairs(pairs: Sequence[Sequence[Tuple[int, int]]], time: int) -> Tuple[torch.Tensor, int]:
    """The chunk table of ``svt_drop_freq_chunk``: ``(B, max_chunks, 2)`` int64 on the CPU and ``max_chunks`` (0: no clip has a chunk).
    Every pair goes through Python's slice rules for a row of ``time`` samples, which is what the reference's ``x[i, start:end] = 0``
    applies: an end behind the row is cut there, negative indices count from the end.  Rows with fewer chunks fill up with (0, 0)."""
    most = max((len(p) for p in pairs), default=0)
    table = torch.zeros((len(pairs), max(most, 1), 2), dtype=torch.int64)
    for i, row in enumerate(pairs):
        for j, (start, end) in enumerate(row):
            lo, hi, _ = slice(start, end).indices(time)
            table[i, j, 0], table[i, j, 1] = lo, hi
    return table, most


class _Staging:
    """Pinned host buffers for a call's tables -- the filter's taps in the first 64 words, the chunk pairs behind them -- which go up in
    ONE asynchronous copy.  Four buffers take turns, and one is rewritten only after the copy of its previous turn has left it (an
    event), so the host does not wait for the stream unless it runs four calls ahead."""
    FILTER_WORDS = 64   # int64 words: 128 floats >= FILTER_LENGTH
    SLOTS = 4

    def __init__(self):
        self.slots = [None] * self.SLOTS   # (pinned buffer, event of its last copy)
        self.turn = 0

    def upload(self, device, taps: Optional[torch.Tensor], table: Optional[torch.Tensor]):
        """-> (filter on the device or None, chunks on the device or None)."""
        words = self.FILTER_WORDS + (table.numel() if table is not None else 0)
        self.turn = (self.turn + 1) % self.SLOTS
        slot = self.slots[self.turn]
        if slot is not None:
            slot[1].synchronize()
        if slot is None or slot[0].numel() < words:
            slot = self.slots[self.turn] = (torch.empty(max(words, 1024), dtype=torch.int64).pin_memory(), torch.cuda.Event())
        host, event = slot
        if taps is not None:
            host[:self.FILTER_WORDS].view(torch.float32)[:taps.numel()] = taps
        if table is not None:
            host[self.FILTER_WORDS:words] = table.reshape(-1)
        dev = host[:words].to(device, non_blocking=True)
        event.record(torch.cuda.current_stream(device))
        f = dev[:self.FILTER_WORDS].view(torch.float32)[:taps.numel()] if taps is not None else None
        c = dev[self.FILTER_WORDS:] if table is not None else None
        return f, c


def _rows(waveforms: torch.Tensor) -> torch.Tensor:
    """``[batch, time]`` or ``[batch, time, 1]`` on the GPU -> (batch, time) fp32 contiguous."""
    if not torch.is_tensor(waveforms) or not waveforms.is_cuda:
        raise _lib.SvtError("the augmentations need their waveforms on the GPU; there is no CPU fallback")
    if waveforms.dim() == 3:
        if waveforms.shape[2] != 1:
            raise ValueError(f"expected one channel, got {waveforms.shape[2]}: the reference's conv1d against its (1, 1, 101) filter "
                             "cannot take more either")
        waveforms = waveforms[:, :, 0]
    elif waveforms.dim() != 2:
        raise ValueError("Input must be [batch, time] or [batch, time, 1]")
    return waveforms.detach().to(torch.float32).contiguous()


def _launch(x: torch.Tensor, taps: Optional[torch.Tensor], table: Optional[torch.Tensor], max_chunks: int, staging: _Staging) -> torch.Tensor:
    """x (B, T) fp32 contiguous on the GPU; taps (n,) fp32 on the CPU or None; table (B, max_chunks, 2) int64 on the CPU or None."""
    out = torch.empty_like(x)
    if not x.numel():
        return out
    f, c = staging.upload(x.device, taps, table)
    lib = _lib.load()
    _lib.check(lib.svt_drop_freq_chunk(_lib.ptr(x), x.shape[0], x.shape[1], x.shape[1], _lib.ptr(f) if f is not None else None,
                                       taps.numel() if taps is not None else 0, _lib.ptr(c) if c is not None else None,
                                       max_chunks if c is not None else 0, _lib.ptr(out), x.shape[1], _lib.dev_index(x.device),
                                       _lib.stream_ptr(x.device)), "svt_drop_freq_chunk")
    return out


class DropFreq(torch.nn.Module):
    """``speechbrain.processing.speech_augmentation.DropFreq``: ``drop_count`` random frequencies (fractions of half the sampling rate)
    notched out of the whole batch by one 101-tap filter.  ``[batch, time]`` -> ``[batch, time]``; ``[batch, time, 1]`` comes back as
    ``[batch, time]`` when the filter ran and as a ``[batch, time, 1]`` clone when ``drop_prob`` missed, as in the reference (its final
    ``squeeze(-1)``).  A miss or a count of zero (the reference then convolves with a delta) returns a clone without a launch.
    ``self.frequencies`` / ``self.filter`` hold the last call's draws and taps (None after a miss)."""

    def __init__(self, drop_freq_low=1e-14, drop_freq_high=1, drop_count_low=1, drop_count_high=2, drop_width=0.05, drop_prob=1):
        super().__init__()
        self.drop_freq_low, self.drop_freq_high = drop_freq_low, drop_freq_high
        self.drop_count_low, self.drop_count_high = drop_count_low, drop_count_high
        self.drop_width, self.drop_prob = drop_width, drop_prob
        self.frequencies = self.filter = None
        self._staging = _Staging()

    def draw(self) -> Optional[torch.Tensor]:
        """The call's draws; the taps (or None: nothing to filter) are left in ``self.filter``."""
        self.frequencies = draw_frequencies(self.drop_freq_low, self.drop_freq_high, self.drop_count_low, self.drop_count_high, self.drop_prob)
        fired = self.frequencies is not None and self.frequencies.numel() > 0
        self.filter = drop_filter(self.frequencies, self.drop_width) if fired else None
        return self.frequencies

    @torch.no_grad()
    def forward(self, waveforms: torch.Tensor) -> torch.Tensor:
        x = _rows(waveforms)
        if self.draw() is None:
            return waveforms.clone()
        if self.filter is None:
            return x.clone() if x.data_ptr() == waveforms.data_ptr() else x
        return _launch(x, self.filter, None, 0, self._staging)


class DropChunk(torch.nn.Module):
    """``speechbrain.processing.speech_augmentation.DropChunk``: ``drop_count`` spans of ``drop_length`` samples zeroed per clip, with
    the reference's validation and its clamping of the length limits to ``drop_end - drop_start``.  ``lengths``: the clips' relative
    lengths, ``[batch]``; on the CPU they cost nothing, on the GPU one device-to-host copy of the B values (the spans are drawn on the
    host from them).  ``noise_factor`` must be 0: the reference draws that noise with one ``torch.rand(length, device=...)`` per chunk
    from the DEVICE generator, and reproducing it means either those B x count launches or a different stream of numbers.
    ``self.chunks`` holds the last call's ``(start, end)`` pairs per clip (None after a miss)."""

    def __init__(self, drop_length_low=100, drop_length_high=1000, drop_count_low=1, drop_count_high=10, drop_start=0, drop_end=None,
                 drop_prob=1, noise_factor=0.0):
        super().__init__()
        self.drop_length_low, self.drop_length_high = drop_length_low, drop_length_high
        self.drop_count_low, self.drop_count_high = drop_count_low, drop_count_high
        self.drop_start, self.drop_end, self.drop_prob, self.noise_factor = drop_start, drop_end, drop_prob, noise_factor
        if drop_length_low > drop_length_high:
            raise ValueError("Low limit must not be more than high limit")
        if drop_count_low > drop_count_high:
            raise ValueError("Low limit must not be more than high limit")
        if drop_end is not None and drop_end >= 0:
            if drop_start > drop_end:
                raise ValueError("Low limit must not be more than high limit")
            drop_range = drop_end - drop_start
            self.drop_length_low = min(drop_length_low, drop_range)
            self.drop_length_high = min(drop_length_high, drop_range)
        if noise_factor:
            raise NotImplementedError("noise_factor != 0 is not supported: the reference fills each chunk from one torch.rand(length) on "
                                      "the device generator, which one launch cannot reproduce draw for draw; use 0 (the lobe's default)")
        self.chunks = None
        self._staging = _Staging()

    def draw(self, lengths: torch.Tensor, time: int):
        """The call's draws for clips of relative ``lengths`` in rows of ``time`` samples: ``(table, max_chunks)`` of ``slice_pairs``, or
        ``(None, 0)`` when nothing is dropped."""
        self.chunks = draw_chunks(sample_lengths(lengths, time), self.drop_length_low, self.drop_length_high, self.drop_count_low,
                                  self.drop_count_high, self.drop_start, self.drop_end, self.drop_prob)
        if self.chunks is None:
            return None, 0
        table, most = slice_pairs(self.chunks, time)
        return (table, most) if most else (None, 0)

    @torch.no_grad()
    def forward(self, waveforms: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
        x = _rows(waveforms)
        table, most = self.draw(lengths, x.shape[1])
        if table is None:
            return waveforms.clone()
        return _launch(x, None, table, most, self._staging).view(waveforms.shape)


class TimeDomainSpecAugment(torch.nn.Module):
    """``speechbrain.lobes.augment.TimeDomainSpecAugment``: speed perturbation, frequency dropping and chunk dropping, with the lobe's
    constructor.  ``forward(waveforms, lengths)`` launches ``SpeedPerturb`` (a resampling, unless the drawn speed is 100) and then ONE
    ``svt_drop_freq_chunk`` with both the filter and the chunk table; when neither fires, a clone.  The draws come in the reference's
    order: the speed, the frequencies, then the chunks for the length the speed step left.  Shapes as in the reference: ``[batch,
    time]`` -> ``[batch, time']``; ``[batch, time, 1]`` loses its channel axis whenever ``DropFreq`` fires.  ``lengths`` as in
    ``DropChunk``."""

    def __init__(self, perturb_prob=1.0, drop_freq_prob=1.0, drop_chunk_prob=1.0, speeds=[95, 100, 105], sample_rate=16000,
                 drop_freq_count_low=0, drop_freq_count_high=3, drop_chunk_count_low=0, drop_chunk_count_high=5,
                 drop_chunk_length_low=1000, drop_chunk_length_high=2000, drop_chunk_noise_factor=0):
        super().__init__()
        self.speed_perturb = SpeedPerturb(perturb_prob=perturb_prob, orig_freq=sample_rate, speeds=speeds)
        self.drop_freq = DropFreq(drop_prob=drop_freq_prob, drop_count_low=drop_freq_count_low, drop_count_high=drop_freq_count_high)
        self.drop_chunk = DropChunk(drop_prob=drop_chunk_prob, drop_count_low=drop_chunk_count_low, drop_count_high=drop_chunk_count_high,
                                    drop_length_low=drop_chunk_length_low, drop_length_high=drop_chunk_length_high,
                                    noise_factor=drop_chunk_noise_factor)
        self.perturbed = None   # the last call's SpeedPerturb output, (batch, time') fp32
        self._staging = _Staging()

    @torch.no_grad()
    def forward(self, waveforms: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
        _rows(waveforms)                                    # the refusals, before anything is drawn
        y = self.speed_perturb(waveforms)
        x = self.perturbed = _rows(y)
        squeezed = self.drop_freq.draw() is not None        # the reference's DropFreq ends in squeeze(-1) once drop_prob has hit
        shape = x.shape if squeezed else y.shape
        table, most = self.drop_chunk.draw(lengths, x.shape[1])
        taps = self.drop_freq.filter
        if taps is None and table is None:
            out = x if x.data_ptr() != waveforms.data_ptr() else x.clone()
            return out.view(shape)
        return _launch(x, taps, table, most, self._staging).view(shape)
