"""Host side of the video recipe's training input: ``TrainTransform`` against what the reference's own ``transform_train`` drew and
computed (tests/golden/video_train.pt, written by tests/golden/make_golden_video_train.py), ``EvalTransform.plan`` and
``pad_roi_batch``.  No GPU."""
import random

import numpy as np
import pytest
import torch

import svt_speechbrain_amd as S
from svt_speechbrain_amd.video import TrainTransform, EvalTransform, VideoClip, pad_roi_batch

CASES = ["roi96_noflip", "roi96_flip", "roi97x99_odd", "roi88", "crop60"]


def _tf(fx, **kw):
    return TrainTransform(crop=(fx["crop"], fx["crop"]), **kw)


def test_the_fixture_covers_what_it_says(golden):
    fx = golden("video_train")
    assert sorted(fx) == sorted(CASES)
    assert fx["roi96_noflip"]["draw"][2] is False and fx["roi96_flip"]["draw"][2] is True
    dy, dx, _ = fx["roi97x99_odd"]["draw"]
    assert tuple(fx["roi97x99_odd"]["roi"].shape[1:]) == (97, 99) and dy % 2 == 1 and dx % 2 == 1
    assert tuple(fx["roi88"]["roi"].shape[1:]) == (88, 88) and fx["roi88"]["draw"][:2] == (0, 0)
    assert fx["crop60"]["crop"] == 60


@pytest.mark.parametrize("name", CASES)
def test_draw_is_the_references_draw_and_leaves_its_random_state(golden, name):
    fx = golden("video_train")[name]
    h, w = fx["roi"].shape[1:]
    random.seed(fx["seed"])
    assert _tf(fx).draw(h, w) == tuple(fx["draw"])
    assert random.getstate() == fx["state_after"]
    # a generator of its own: same numbers, the module's state untouched
    before = random.getstate()
    assert _tf(fx, rng=random.Random(fx["seed"])).draw(h, w) == tuple(fx["draw"])
    assert random.getstate() == before


@pytest.mark.parametrize("name", CASES)
def test_host_transform_equals_the_reference_in_every_bit(golden, name):
    fx = golden("video_train")[name]
    random.seed(fx["seed"])
    got = _tf(fx)(fx["roi"].numpy())                                     # draws for itself
    assert got.dtype == np.float32 and random.getstate() == fx["state_after"]
    assert np.array_equal(got.view(np.int32), fx["sig"].numpy().view(np.int32))
    state = random.getstate()
    again = _tf(fx)(fx["roi"].numpy(), draw=tuple(fx["draw"]))           # a given draw consumes nothing
    assert np.array_equal(again.view(np.int32), got.view(np.int32)) and random.getstate() == state


def test_flip_ratio_zero_never_flips_and_one_always_does():
    r = random.Random(11)
    never, always = TrainTransform(flip_ratio=0.0, rng=r), TrainTransform(flip_ratio=1.0, rng=r)
    assert not any(never.draw(96, 96)[2] for _ in range(200))
    assert all(always.draw(96, 96)[2] for _ in range(200))
    roi = np.arange(2 * 96 * 96, dtype=np.int64).reshape(2, 96, 96).astype(np.uint8)
    a, b = always(roi, draw=(3, 5, False)), always(roi, draw=(3, 5, True))
    assert np.array_equal(a[..., ::-1], b) and not np.array_equal(a, b)


def test_a_roi_smaller_than_the_crop_raises():
    tf = TrainTransform(rng=random.Random(1))
    state = tf.rng.getstate()
    for h, w in [(87, 96), (96, 87), (80, 80)]:
        with pytest.raises(ValueError):
            tf.draw(h, w)
        with pytest.raises(ValueError):
            tf(np.zeros((1, h, w), dtype=np.uint8))
        with pytest.raises(ValueError):
            tf.plan([1], h, w)
    assert tf.rng.getstate() == state                                    # refused before anything is drawn
    with pytest.raises(ValueError):
        tf(np.zeros((1, 96, 96), dtype=np.uint8), draw=(9, 0, False))    # an offset outside the frame


def test_plan_consumes_one_draw_per_clip_in_batch_order():
    tf = TrainTransform(rng=random.Random(7))
    plan = tf.plan([12, 9, 5], 96, 98)
    ref, single = random.Random(7), TrainTransform(rng=random.Random(7))
    want = []
    for n in (12, 9, 5):
        dx = ref.randint(0, 98 - 88)
        dy = ref.randint(0, 96 - 88)
        want.append(VideoClip(dy, dx, int(ref.random() < 0.5), n))
    assert plan == want and [single.draw(96, 98) for _ in range(3)] == [(c.dy, c.dx, bool(c.flip)) for c in plan]
    assert tf.rng.getstate() == ref.getstate() == single.rng.getstate()  # exactly three draws
    assert all(isinstance(c, VideoClip) and type(c.flip) is int for c in plan)


def test_eval_plan_is_the_centre_crop_without_a_flip_and_draws_nothing():
    state = random.getstate()
    assert EvalTransform().plan([6, 2], 97, 99) == [VideoClip(4, 5, 0, 6), VideoClip(4, 5, 0, 2)]
    assert EvalTransform().plan([3], 96, 96) == [VideoClip(4, 4, 0, 3)] and EvalTransform().offsets(97, 99) == (4, 5)
    assert random.getstate() == state
    with pytest.raises(ValueError):
        EvalTransform().plan([3], 80, 96)


def test_pad_roi_batch():
    g = torch.Generator().manual_seed(2)
    clips = [torch.randint(0, 256, (t, 10, 12), generator=g, dtype=torch.uint8) for t in (3, 5, 1)]
    roi, lengths = pad_roi_batch(clips)
    assert roi.shape == (3, 5, 10, 12) and roi.dtype == torch.uint8 and lengths == [3, 5, 1]
    for b, c in enumerate(clips):
        assert torch.equal(roi[b, :lengths[b]], c)
    with pytest.raises(ValueError):
        pad_roi_batch(clips + [torch.zeros((2, 10, 13), dtype=torch.uint8)])
    with pytest.raises(ValueError):
        pad_roi_batch(clips + [torch.zeros((2, 11, 12), dtype=torch.uint8)])
    with pytest.raises(ValueError):
        pad_roi_batch([torch.zeros((2, 10, 12))])
    with pytest.raises(ValueError):
        pad_roi_batch([])


def test_exports():
    for name in ("TrainTransform", "VideoClip", "pad_roi_batch", "VideoProbe"):
        assert name in S.__all__ and hasattr(S, name)
    assert issubclass(S.VideoProbe, S.LinearProbe)
