"""The host side of ``apply_spec_augment=True``: the mask draws of HF's ``_compute_mask_indices`` and their way to the device.

HF's ``_mask_hidden_states`` (``transformers`` ``modeling_wav2vec2.py``; the HuBERT, WavLM and data2vec-audio models carry copies)
draws a ``(B, T)`` time mask and then a ``(B, D)`` feature mask from numpy's GLOBAL generator on the host.  ``compute_mask_indices``
consumes that generator exactly as HF does without an attention mask -- one ``np.random.rand(1)`` for the rounding epsilon, then one
``np.random.choice(np.arange(L - (mask_length - 1)), n, replace=False)`` per batch row -- so a run seeded alike draws the same masks
and leaves the generator in the same state.  The reference never passes an attention mask, so none is supported and
padded frames can be masked, as there.  The masks are applied on the GPU by ``svt_spec_augment`` (``csrc/spec_augment.hip``) inside
the encoder's forward: ``HuggingFaceWav2Vec2`` uploads them through ``MaskStaging``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch


def compute_mask_indices(shape: Tuple[int, int], mask_prob: float, mask_length: int, min_masks: int = 0) -> np.ndarray:
    """HF ``_compute_mask_indices(shape, mask_prob, mask_length, attention_mask=None, min_masks=min_masks)``: a bool ``shape`` array
    with ``mask_prob * shape[1] / mask_length`` (probabilistically rounded, at least ``min_masks``, at most ``shape[1] //
    mask_length``) spans of ``mask_length`` set per row; spans may overlap.  The draws, their order and their arguments are HF's."""
    batch_size, sequence_length = shape
    if mask_length < 1:
        raise ValueError("`mask_length` has to be bigger than 0.")
    if mask_length > sequence_length:
        raise ValueError(f"`mask_length` has to be smaller than `sequence_length`, but got `mask_length`: {mask_length}"
                         f" and `sequence_length`: {sequence_length}`")
    epsilon = np.random.rand(1).item()   # probabilistic rounding
    num_masked_span = max(int(mask_prob * sequence_length / mask_length + epsilon), min_masks)
    if num_masked_span * mask_length > sequence_length:          # the clamp
        num_masked_span = sequence_length // mask_length
    if sequence_length - (mask_length - 1) < num_masked_span:
        num_masked_span = max(sequence_length - (mask_length - 1), 0)
    mask = np.zeros((batch_size, sequence_length), dtype=bool)
    if num_masked_span == 0:
        return mask
    # without an attention mask every row has the full length: the same span count, so HF's dummy-index padding adds nothing
    starts = np.empty((batch_size, num_masked_span), dtype=np.int64)
    for b in range(batch_size):
        starts[b] = np.random.choice(np.arange(sequence_length - (mask_length - 1)), num_masked_span, replace=False)
    idx = (starts[:, :, None] + np.arange(mask_length)[None, None, :]).reshape(batch_size, -1)
    np.minimum(idx, sequence_length - 1, out=idx)
    np.put_along_axis(mask, idx, True, -1)
    return mask


def draw_masks(cfg, B: int, T: int) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
    """The two draws of ``_mask_hidden_states`` in training mode, in its order: the ``(B, T)`` time mask, then the ``(B, D)`` feature
    mask, each only when its probability is above 0 (None otherwise: no draw, the generator is not touched)."""
    tm = fm = None
    if cfg.mask_time_prob > 0:
        tm = compute_mask_indices((B, T), cfg.mask_time_prob, cfg.mask_time_length, cfg.mask_time_min_masks)
    if cfg.mask_feature_prob > 0:
        fm = compute_mask_indices((B, cfg.hidden_size), cfg.mask_feature_prob, cfg.mask_feature_length, cfg.mask_feature_min_masks)
    return tm, fm


def generator_digest() -> str:
    """sha256 of numpy's global generator state (MT19937 key, position and the cached-normal fields): what the fixtures record."""
    import hashlib
    name, key, pos, has_gauss, gauss = np.random.get_state()
    h = hashlib.sha256()
    h.update(name.encode())
    h.update(np.ascontiguousarray(key, dtype=np.uint32).tobytes())
    h.update(np.array([pos, has_gauss], dtype=np.int64).tobytes())
    h.update(np.array([gauss], dtype=np.float64).tobytes())
    return h.hexdigest()


class MaskStaging:
    """Pinned host buffers for a forward's two masks, which go up in ONE asynchronous copy (``augment._Staging`` is the precedent).
    Four buffers take turns, and one is rewritten only after the copy of its previous turn has left it (an event), so the host does
    not wait for the stream unless it runs four forwards ahead.  The feature mask starts at a 16-byte boundary behind the time mask."""
    SLOTS = 4

    def __init__(self):
        self.slots = [None] * self.SLOTS   # (pinned buffer, event of its last copy)
        self.turn = 0

    def upload(self, device, time_mask: Optional[np.ndarray], feature_mask: Optional[np.ndarray]):
        """-> (time mask on the device or None, feature mask on the device or None), uint8."""
        nt = time_mask.size if time_mask is not None else 0
        off = (nt + 15) // 16 * 16
        n = off + (feature_mask.size if feature_mask is not None else 0)
        self.turn = (self.turn + 1) % self.SLOTS
        slot = self.slots[self.turn]
        if slot is not None:
            slot[1].synchronize()
        if slot is None or slot[0].numel() < n:
            slot = self.slots[self.turn] = (torch.empty(max(n, 65536), dtype=torch.uint8).pin_memory(), torch.cuda.Event())
        host, event = slot
        view = host.numpy()
        if time_mask is not None:
            view[:nt] = time_mask.reshape(-1)
        if feature_mask is not None:
            view[off:n] = feature_mask.reshape(-1)
        dev = host[:n].to(device, non_blocking=True)
        event.record(torch.cuda.current_stream(device))
        return (dev[:nt] if time_mask is not None else None), (dev[off:n] if feature_mask is not None else None)
