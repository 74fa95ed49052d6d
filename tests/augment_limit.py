"""What tests/test_augment_limit.py (CPU) and tests/test_gpu_augment.py (GPU) share: the exact (fp64) correlation of a waveform batch with
an fp32 filter, the per-element limit a correct fp32 evaluation stays inside, such an evaluation with its mutants, the chunk rule, the
fp64 build of DropFreq's filter, and the fixture tests/golden/augment.pt (tests/golden/make_golden_augment.py wrote it by running the
reference's own DropFreq, DropChunk and TimeDomainSpecAugment; no test reads the reference).

The sum (speechbrain/processing/speech_augmentation.py:958-974 through conv1d), with h = taps // 2:

    y[t] = sum_{k < taps} f[k] x[t + k - h]            x = 0 outside [0, n)

The limit is a bound, not a fitted tolerance.  With M = sum_k |f[k] x[t + k - h]| in fp64,

    limit = (taps + 1) * 2^-24 * M + 2^-149

counts the roundings of ANY fp32 evaluation of the taps-term sum, fused or not, in any order: `taps` products and taps - 1 additions, each
rounded once by at most 2^-24 of a partial sum that never exceeds M (to first order), and one unit to spare for the second-order terms;
2^-149 is half the spacing of fp32's subnormals.  It is the count of tests/resample_limit.py.

Measured on the CPU with dense Gaussian taps and Gaussian input at 0.25, n = 3 .. 5003, in units of the limit: torch's conv1d 0.007 -
0.035, a plain ascending fp32 sum 0.010 - 0.033, descending 0.007 - 0.039; the reference's DropFreq on its own filter 0.078; the mutants
(window shifted by one, taps flipped, bf16 taps, edges clamped instead of zero-padded, first or last tap dropped at n >= 101) 11 - 9.5e5.
The dropped-tap mutants are invisible at n <= 50, where those taps only meet padding, and on the reference's own filters, whose end taps
are ~0: hence dense taps at n >= 101."""
import hashlib
import os

import torch

from resample_limit import seeded_input, sha256, worst  # noqa: F401  (the same seeded Gaussian input, digest and ratio)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment.pt")
TAPS = 101

# the fixture's cases: name -> (kind, constructor arguments, input shape, relative lengths or None, seed of the draws)
CASES = {
    "drop_freq_1": ("DropFreq", dict(drop_count_low=1, drop_count_high=1), (2, 1500), None, 101),
    "drop_freq_2": ("DropFreq", dict(drop_count_low=2, drop_count_high=2), (2, 1500), None, 102),
    "drop_chunk": ("DropChunk", dict(), (3, 3000), (1.0, 0.5, 0.03), 103),              # the third clip, 90 samples, is shorter than its chunks
    "drop_chunk_negative": ("DropChunk", dict(drop_start=-2000, drop_end=-100, drop_length_low=100, drop_length_high=500), (3, 3000),
                            (1.0, 0.9, 0.8), 104),
    "lobe_100": ("TimeDomainSpecAugment", dict(speeds=[100]), (3, 6000), (1.0, 0.75, 0.5), 105),
    "lobe_speeds": ("TimeDomainSpecAugment", dict(speeds=[95, 100, 105]), (3, 6000), (1.0, 0.75, 0.5), 119),   # this seed draws 105 %
}


def case_input(name):
    kind, kwargs, shape, lengths, seed = CASES[name]
    return seeded_input(shape[0], shape[1], 7000 + seed)


def case_lengths(name):
    lengths = CASES[name][3]
    return None if lengths is None else torch.tensor(lengths, dtype=torch.float32)


def load_fixture():
    return torch.load(GOLDEN, weights_only=False)


def rng_digest():
    """sha256 of the CPU default generator's state: equal digests, equal draws so far."""
    return hashlib.sha256(torch.get_rng_state().numpy().tobytes()).hexdigest()


def dense_taps(taps, seed):
    """Gaussian taps: every tap matters, the end ones included."""
    return torch.randn(taps, generator=torch.Generator().manual_seed(seed)) / taps ** 0.5


def _windows(x, taps, clamp=False, shift=0):
    """(rows, n, taps): x[t + k - taps // 2 + shift], zero (clamp: the nearest edge sample) outside [0, n)."""
    n = x.shape[1]
    idx = torch.arange(n).unsqueeze(1) + torch.arange(taps).unsqueeze(0) - taps // 2 + shift
    inside = (idx >= 0) & (idx < n)
    win = x[:, idx.clamp(0, n - 1)]
    return win if clamp else torch.where(inside, win, torch.zeros((), dtype=x.dtype))


def exact(x, f):
    """(y, M): the fp64 correlation of x (rows, n) fp32 with the fp32 taps f and the magnitude sum, (rows, n) each.  conv1d in fp64 (a
    cross-correlation by definition; its own rounding, 2^-53 a term, is nothing against the limit), one row at a time to stay small."""
    h = f.numel() // 2
    w = f.double().view(1, 1, -1)
    xd = x.double().unsqueeze(1)
    with torch.no_grad():
        return (torch.nn.functional.conv1d(xd, w, padding=h)[:, 0], torch.nn.functional.conv1d(xd.abs(), w.abs(), padding=h)[:, 0])


def exact_by_windows(x, f):
    """The same two sums written out term by term (small inputs: rows x n x taps values)."""
    terms = _windows(x.double(), f.numel()) * f.double()
    return terms.sum(-1), terms.abs().sum(-1)


def limit(M, taps):
    return (taps + 1) * 2.0 ** -24 * M + 2.0 ** -149


def chunk_mask(pairs, rows, n):
    """(rows, n) bool: t with start <= t < end for any (start, end) of the row; end > n is cut at n, start >= end is empty."""
    mask = torch.zeros((rows, n), dtype=torch.bool)
    for r, row in enumerate(pairs):
        for start, end in row:
            start, end = max(0, min(n, int(start))), max(0, min(n, int(end)))
            if start < end:
                mask[r, start:end] = True
    return mask


MUTANTS = ("window_shifted", "flipped_taps", "bf16_taps", "edge_clamped", "first_tap_dropped", "last_tap_dropped")


def direct_fp32(x, f, mutant=None, descending=False):
    """A correct evaluation -- every product rounded to fp32 and added in ascending (or descending) tap order in fp32 -- or a mutant of
    it: the window one sample off, the taps flipped (convolution where correlation belongs), taps rounded to bf16, edge samples repeated
    where zeros belong, the first or the last tap left out."""
    assert mutant is None or mutant in MUTANTS
    taps = f.numel()
    f = f.float()
    if mutant == "flipped_taps":
        f = f.flip(0)
    if mutant == "bf16_taps":
        f = f.bfloat16().float()
    win = _windows(x.float(), taps, clamp=mutant == "edge_clamped", shift=1 if mutant == "window_shifted" else 0)
    order = list(range(taps))
    if mutant == "first_tap_dropped":
        order = order[1:]
    if mutant == "last_tap_dropped":
        order = order[:-1]
    if descending:
        order = order[::-1]
    acc = torch.zeros(win.shape[:2], dtype=torch.float32)
    for k in order:
        acc = acc + win[:, :, k] * f[k]
    return acc


def notch_filter_fp64(notch_freq, filter_width=TAPS, notch_width=0.05):
    """The formulas of notch_filter in fp64: sinc low-pass at notch_freq and high-pass at notch_freq + 2 notch_width under the periodic
    Blackman window, each normalised by its sum."""
    pad = filter_width // 2
    t = (torch.arange(filter_width) - pad).double()
    window = torch.blackman_window(filter_width, dtype=torch.float64)
    centre = float(notch_freq) + notch_width

    def sinc(a):
        safe = torch.where(a == 0, torch.ones_like(a), a)
        return torch.where(a == 0, torch.ones_like(a), torch.sin(safe) / safe)

    lp = sinc(3 * (centre - notch_width) * t) * window
    lp = lp / lp.sum()
    hp = sinc(3 * (centre + notch_width) * t) * window
    hp = hp / -hp.sum()
    hp[pad] += 1
    return lp + hp


def drop_filter_fp64(frequencies, drop_width=0.05):
    """The compound filter in fp64 at the given (fp32) frequencies: a delta cross-correlated with one notch after the other, 50 zeros
    either side, as conv1d does it."""
    pad = TAPS // 2
    f = torch.zeros(TAPS, dtype=torch.float64)
    f[pad] = 1
    for frequency in torch.as_tensor(frequencies, dtype=torch.float32).reshape(-1):
        kernel = notch_filter_fp64(frequency, TAPS, drop_width)
        f = (_windows(f.unsqueeze(0), TAPS) * kernel).sum(-1)[0]
    return f
