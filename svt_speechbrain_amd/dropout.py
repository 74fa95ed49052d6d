"""Host side of the encoder's training-mode layerdrop (HF modeling_wav2vec2.py, the encoder loops): the draws, made exactly as HF makes
them, so a run seeded alike skips the same layers and leaves torch's host generator in the same state.  The element dropouts have no
host part: their mask is a function of position computed on the device (csrc/dropout.hip, include/svt_mi355.h "svt_dropout")."""
from __future__ import annotations

from typing import Tuple

import torch


def draw_layerdrop(num_layers: int, layerdrop: float, family: str = "wav2vec2") -> Tuple[bool, ...]:
    """One ``torch.rand([])`` per layer, in layer order, from torch's HOST default generator; layer ``l`` is skipped iff its draw is
    ``< layerdrop``.  HF draws whatever ``layerdrop`` is (0 included), so this does too.  HF's WavLM encoder draws for layer 0 like for
    the others but never skips it (``i > 0``): only that layer holds the position embedding."""
    skipped = []
    for l in range(int(num_layers)):
        below = bool(torch.rand([]) < layerdrop)
        skipped.append(below and not (family == "wavlm" and l == 0))
    return tuple(skipped)
