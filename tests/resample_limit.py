"""What tests/test_resample_limit.py (CPU) and tests/test_gpu_resample.py (GPU) share: the exact (fp64) polyphase sum over the fp32 filter
table, the per-element limit a correct fp32 evaluation stays inside, such an evaluation with its mutants, and the fixture
tests/golden/resample.pt (tests/golden/make_golden_resample.py wrote it by running the reference's own Resample class; no test reads the
reference).

The sum (speechbrain/processing/speech_augmentation.py:479-789), with S input samples and P outputs per unit:

    y[n P + p] = sum_{j < W} x[n S + first[p] + j] w[p][j]            x = 0 outside [0, n_in)

The limit is a bound, not a fitted tolerance.  With M = sum_j |x_j w_j| in fp64,

    limit = (W + 1) * 2^-24 * M + 2^-149

counts the roundings of ANY fp32 evaluation of the W-term sum, fused or not, in any order: W products and W - 1 additions, each rounded
once by at most 2^-24 of a partial sum that never exceeds M (to first order), and one unit to spare for the second-order terms; 2^-149 is
half the spacing of fp32's subnormals.  Downmix, 0.5 (y_0 + y_1): one more addition (the halving is exact) over twice the terms,

    limit = (W + 2) * 2^-24 * 0.5 * sum_c sum_j |x_{c,j} w_j| + 2^-149

The reference's own output (conv1d per phase on the CPU) reaches 0.01 - 0.31 of it on Gaussian input, a plain ascending fp32 sum
0.01 - 0.33: against the recorded reference outputs the kernel is held to (1 + ref_vs_fp64) * limit by the triangle inequality,
ref_vs_fp64 being the recorded distance of the reference from the exact sum in units of the limit."""
import hashlib
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample.pt")
# the recipes' sources (44.1 / 48 / 22.05 kHz -> 16 kHz), SpeedPerturb at 95 and 105 % of 16 kHz, and one upsampling with P > S
RATIOS = ((44100, 16000), (48000, 16000), (22050, 16000), (16000, 15200), (16000, 16800), (16000, 44100))
LENGTHS = (3, 441, 5003)
N_OUT_LENGTHS = 2000   # n_out is recorded for input lengths 1 .. 2000


def load_fixture():
    return torch.load(GOLDEN, weights_only=False)


def sha256(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def seeded_input(rows, n, seed):
    """(rows, n) Gaussian at 0.25: every sample non-zero, the edges included."""
    return 0.25 * torch.randn(rows, n, generator=torch.Generator().manual_seed(seed))


def input_seed(orig, new, n):
    return 9000 + (orig // 50 + new // 100 + n) % 1000


def tick_rule(n_in, P, S):
    """n_out of n_in input samples: the outputs at ticks in [0, n_in P), one every S ticks."""
    interval = n_in * P
    if interval <= 0:
        return 0
    last = interval // S
    return last if last * S == interval else last + 1


def _windows(x, first, P, W, S, n_out, clamp=False):
    """(rows, n_out, W): x[n S + first[p] + j] for every output n P + p, zero (or, clamp: the nearest edge sample) outside [0, n_in)."""
    o = torch.arange(n_out)
    n, p = o // P, o % P
    idx = (n * S + first.long()[p]).unsqueeze(1) + torch.arange(W).unsqueeze(0)
    inside = (idx >= 0) & (idx < x.shape[1])
    win = x[:, idx.clamp(0, x.shape[1] - 1)]
    return (win if clamp else torch.where(inside, win, torch.zeros((), dtype=x.dtype))), p


def exact(x, first, weights, S, n_out):
    """(y, M): the fp64 sum over the fp32 table and the magnitude sum sum_j |x_j w_j|, (rows, n_out) each, of x (rows, n_in) fp32."""
    P, W = weights.shape
    win, p = _windows(x.double(), first, P, W, S, n_out)
    terms = win * weights.double()[p]
    return terms.sum(-1), terms.abs().sum(-1)


def limit(M, W):
    return (W + 1) * 2.0 ** -24 * M + 2.0 ** -149


def downmix_exact(y, M):
    """(0.5 (y_0 + y_1), 0.5 (M_0 + M_1)) of consecutive row pairs."""
    return 0.5 * (y[0::2] + y[1::2]), 0.5 * (M[0::2] + M[1::2])


def downmix_limit(M_half, W):
    """M_half = 0.5 * sum_c sum_j |x_{c,j} w_j| (downmix_exact's second result)."""
    return (W + 2) * 2.0 ** -24 * M_half + 2.0 ** -149


def worst(got, ref, lim):
    """Largest |got - ref| / limit; a NaN or an infinity anywhere counts as infinite."""
    r = (got.double() - ref).abs() / lim
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    return r.max().item() if r.numel() else 0.0


MUTANTS = ("first_plus_1", "first_minus_1", "last_tap_dropped", "next_phase_row", "stride_plus_1", "stride_minus_1", "edge_clamped",
           "bf16_weights", "sum_not_halved")


def direct_fp32(x, first, weights, S, n_out, mutant=None, downmix=False):
    """A correct evaluation -- every product rounded to fp32 and added in ascending tap order in fp32 -- or a mutant of it: first[] off by
    one either way, the last tap dropped, phase p with the filter of phase p + 1 (P > 1), a unit stride of S +- 1, edge samples repeated
    where zeros belong, weights rounded to bf16, and (downmix) the two channels summed without the halving."""
    assert mutant is None or mutant in MUTANTS
    P, W = weights.shape
    first = first + {"first_plus_1": 1, "first_minus_1": -1}.get(mutant, 0)
    S = S + {"stride_plus_1": 1, "stride_minus_1": -1}.get(mutant, 0)
    if mutant == "bf16_weights":
        weights = weights.bfloat16().float()
    win, p = _windows(x.float(), first, P, W, S, n_out, clamp=mutant == "edge_clamped")
    w = weights[(p + 1) % P] if mutant == "next_phase_row" else weights[p]
    acc = torch.zeros(win.shape[:2], dtype=torch.float32)
    for j in range(W - 1 if mutant == "last_tap_dropped" else W):
        acc = acc + win[:, :, j] * w[:, j]
    if not downmix:
        return acc
    s = acc[0::2] + acc[1::2]
    return s if mutant == "sum_not_halved" else 0.5 * s
