"""Generate tests/golden/video_train.pt by running the REFERENCE's own ``transform_train``.

Runs only where the reference is checked out (the path ``make_golden.py`` names); the fixture it writes -- data only: uint8
inputs, seeds, the drawn numbers, expected float32 outputs, the state of ``random`` afterwards -- is committed, the reference never is.

    python tests/golden/make_golden_video_train.py

What runs is ``Compose([Normalize(0.0, 255.0), RandomCrop((th, tw)), HorizontalFlip(0.5), Normalize(0.421, 0.165)])`` of
``N20EMv2/video_only/train_video_ssl.py:448-452`` with the classes of ``N20EMv2/video_only/utils.py:22-129``, under ``random.seed(s)``,
followed by the pipeline's ``.astype(np.float32)`` (:474-476).  ``cv2`` -- which that file imports for its video reader and for
``cv2.flip(img, 1)`` -- is stubbed as in ``make_golden.make_video_u8_cases``, with ``flip(img, 1) = img[:, ::-1]``.  What the reference
DREW is read back by replaying the three calls of ``RandomCrop`` / ``HorizontalFlip`` on a second generator with the same seed, and
checked against the result (the crop and the mirror are found in the output).
"""
from __future__ import annotations

import importlib.util
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402

# name, ROI height, ROI width, crop, seed (chosen so that the flip is / is not drawn where the case says so)
CASES = [("roi96_noflip", 96, 96, 88, None), ("roi96_flip", 96, 96, 88, None), ("roi97x99_odd", 97, 99, 88, None),
         ("roi88", 88, 88, 88, 3), ("crop60", 64, 70, 60, 4)]
T = 2


def _replay(seed, h, w, th, tw, flip_ratio=0.5):
    r = random.Random(seed)
    dx = r.randint(0, w - tw)
    dy = r.randint(0, h - th)
    flip = r.random() < flip_ratio
    return dy, dx, flip


def _pick_seed(name, h, w, c):
    for s in range(1, 1000):
        dy, dx, flip = _replay(s, h, w, c, c)
        if name == "roi96_noflip" and not flip:
            return s
        if name == "roi96_flip" and flip:
            return s
        if name == "roi97x99_odd" and dy % 2 == 1 and dx % 2 == 1:
            return s
    raise RuntimeError(name)


def main():
    cv2 = types.ModuleType("cv2")
    cv2.flip = lambda img, code: img[:, ::-1] if code == 1 else (_ for _ in ()).throw(ValueError(code))
    sys.modules["cv2"] = cv2
    spec = importlib.util.spec_from_file_location("ref_video_utils", REF + "/N20EMv2/video_only/utils.py")
    ut = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ut)
    out = {}
    data = np.random.RandomState(87)
    for name, h, w, c, seed in CASES:
        if seed is None:
            seed = _pick_seed(name, h, w, c)
        roi = data.randint(0, 256, size=(T, h, w)).astype(np.uint8)
        transform_train = ut.Compose([ut.Normalize(0.0, 255.0), ut.RandomCrop((c, c)), ut.HorizontalFlip(0.5), ut.Normalize(0.421, 0.165)])
        random.seed(seed)
        sig = transform_train(roi).astype(np.float32)
        state = random.getstate()
        dy, dx, flip = _replay(seed, h, w, c, c)
        # the draw, confirmed on the reference's output: byte -> value is injective, so the window is found by its pixels
        want = ((roi[:, dy:dy + c, dx:dx + c] / 255.0 - 0.421) / 0.165)
        want = (want[:, :, ::-1] if flip else want).astype(np.float32)
        assert sig.shape == (T, c, c) and np.array_equal(sig.view(np.int32), want.view(np.int32)), name
        out[name] = dict(roi=torch.from_numpy(roi.copy()), seed=seed, crop=c, draw=(dy, dx, bool(flip)), sig=torch.from_numpy(sig.copy()),
                         state_after=state)
        print("video_train", name, "seed", seed, "draw", (dy, dx, flip), tuple(sig.shape), float(sig.mean()))
    assert not out["roi96_noflip"]["draw"][2] and out["roi96_flip"]["draw"][2] and out["roi88"]["draw"][:2] == (0, 0)
    torch.save(out, os.path.join(HERE, "video_train.pt"))
    print(os.path.getsize(os.path.join(HERE, "video_train.pt")), "bytes")


if __name__ == "__main__":
    main()
