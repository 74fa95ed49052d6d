"""GPU: the video recipe's training input side -- per-clip crop, flip and length inside the lip front-end's padding pass
(svt_video_forward_u8_clips, csrc/video.hip video_pad*_u8_clips_kernel) and the frozen-encoder step on top of it (VideoProbe).

Nothing here needs a tolerance: every comparison is bitwise, against the host restatement ``TrainTransform.__call__`` (pinned to the
reference's own ``transform_train`` by tests/test_video_train_transform.py) or against a path other tests pin to the reference (the
float entry point, svt_video_forward_u8, LinearProbe.fit_features)."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

import svt_speechbrain_amd as S  # noqa: E402
from svt_speechbrain_amd import _lib  # noqa: E402
from svt_speechbrain_amd import weights as W  # noqa: E402
from svt_speechbrain_amd.huggingface_interface import LIB_VARIANT  # noqa: E402
from svt_speechbrain_amd.video import SubModel, TrainTransform, EvalTransform, VideoClip  # noqa: E402

DEV = "cuda:0"
E = 32
PRECISIONS = ["fp32", "bf16", "fp16", "fp16x3"]
# svt_debug_set key 42 (include/svt_mi355.h): 100 * family + form
FLOAT_FAMILY, U8_FAMILY, CLIPS_FAMILY = 100, 200, 300
GENERIC_F32, GENERIC_16, WIDE_16 = 0, 1, 2


def _form(precision, crop_w):
    """The dispatch condition of csrc/video.hip's launchers, restated: the 16-bit storage modes (bf16, fp16) take the 8-pixels-per-store
    kernel when the padded row Wp is a multiple of 8, else the generic 16-bit one; fp32 and the split-operand modes store fp32.
    svt_video_forward's geometry (api_video.hip, video_geom) makes Wp = round_up(crop_w + 8, 8), a multiple of 8 for EVERY width: a
    50-pixel crop selects the 8-wide kernel too, and no width reaches the generic 16-bit kernel through the C-ABI -- for the existing
    family as for the new one -- so there is no "smallest width that does not" to test instead."""
    if precision not in ("bf16", "fp16"):
        return GENERIC_F32
    wp = (crop_w + 8 + 7) // 8 * 8
    return WIDE_16 if wp % 8 == 0 else GENERIC_16


def _lib_of(precision):
    return _lib.load(LIB_VARIANT.get(precision))


def _model(precision, seed=1):
    m = SubModel(512, E, "prelu", precision=precision, seed=seed)
    return m.to(DEV)


def _roi(B, T, H, Wd, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, T, H, Wd), generator=g, dtype=torch.uint8)


def _host_batch(tf, roi, clips):
    """What the reference hands its model: every clip through the host transform with its draw, zero-padded to T -> (B, 1, T, h, w)."""
    B, T = roi.shape[:2]
    x = torch.zeros((B, 1, T, tf.crop_h, tf.crop_w), dtype=torch.float32)
    for b, c in enumerate(clips):
        x[b, 0, :c.n_frames] = torch.from_numpy(tf(roi[b, :c.n_frames].numpy(), draw=(c.dy, c.dx, bool(c.flip))))
    return x


def _padded_operand(m, B, T, h, w):
    """The first workspace region of an fp32-mode module: the stem's operand [B][T + 4][h + 6][round_up(w + 8, 8)]."""
    slot = m._sync(torch.device(DEV))
    Hp, Wp = h + 6, (w + 8 + 7) // 8 * 8
    torch.cuda.synchronize()
    return slot.ws[:B * (T + 4) * Hp * Wp * 4].view(torch.float32).view(B, T + 4, Hp, Wp).cpu()


THREE = [VideoClip(0, 0, 0, 6), VideoClip(9, 11, 1, 1), VideoClip(4, 3, 1, 4)]


def test_padded_operand_is_the_host_transform_in_every_bit_and_zero_everywhere_else():
    """fp32 mode, 3 clips of 6 frames, 97 x 99 -> 88 x 88: the extreme offsets with a flip and ONE real frame, an interior crop with a
    flip and 4, the origin unflipped at full length.  The module is new and its workspace holds 0xFF bytes (NaN patterns) before the
    first call, which therefore has to write everything it later reads -- the operand's halo, its two leading and trailing time
    planes, the whole frames past a clip's length, and the stage halos."""
    lib = _lib_of("fp32")
    m = _model("fp32")
    roi = _roi(3, 6, 97, 99, seed=1)
    slot = m._sync(torch.device(DEV))
    need = lib.svt_video_workspace_bytes(slot.handle, 3, 6, 88, 88)
    slot.workspace(need, torch.device(DEV)).fill_(0xFF)
    tf = TrainTransform()
    y = m.forward_into(roi.to(DEV), transform=tf, clips=THREE)
    assert lib.svt_debug_set(42, 0) == CLIPS_FAMILY + GENERIC_F32
    assert y.shape == (3, 6, E) and torch.isfinite(y).all()
    vp = _padded_operand(m, 3, 6, 88, 88)
    rest = vp.clone()
    for b, c in enumerate(THREE):
        want = torch.from_numpy(tf(roi[b, :c.n_frames].numpy(), draw=(c.dy, c.dx, bool(c.flip))))
        got = vp[b, 2:2 + c.n_frames, 3:3 + 88, 4:4 + 88]
        assert torch.equal(got.contiguous().view(torch.int32), want.view(torch.int32)), f"clip {b}: the kernel's crop / flip / pixel map differs"
        rest[b, 2:2 + c.n_frames, 3:3 + 88, 4:4 + 88] = 0
    assert not rest.view(torch.int32).any(), "halo, time padding and the frames past a clip's length must be +0.0 in every bit"


SAME_OPERAND_CASES = {
    # name: (ROI height, ROI width, crop, frames, clips)
    "crop88_of_97x99": (97, 99, 88, 6, THREE),
    # dx 0, 1, 2, 3 and 10: every byte alignment of a row start (70-byte rows on top); both flips; lengths 1 .. T
    "crop60_every_alignment": (64, 70, 60, 3, [VideoClip(0, 0, 0, 3), VideoClip(4, 1, 1, 2), VideoClip(1, 2, 0, 1), VideoClip(3, 3, 1, 3),
                                                VideoClip(2, 10, 1, 2)]),
    # a width that is no multiple of 4: the last 8-pixel group of a row is cut after 2 pixels
    "crop50": (64, 70, 50, 3, [VideoClip(14, 20, 1, 3), VideoClip(0, 7, 0, 1), VideoClip(5, 0, 1, 2)]),
}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(SAME_OPERAND_CASES))
def test_clips_path_equals_the_float_path_on_the_host_transformed_frames(name, precision):
    """Same model, two inputs: the raw uint8 batch with its clip table, and the host-transformed, zero-padded float frames through the
    float entry point.  The padded operand is the same, so the features are, in every precision.  Key 42 names the kernel that ran."""
    H, Wd, crop, T, clips = SAME_OPERAND_CASES[name]
    lib = _lib_of(precision)
    m = _model(precision)
    roi = _roi(len(clips), T, H, Wd, seed=H + crop)
    tf = TrainTransform(crop=(crop, crop))
    a = m.forward_into(roi.to(DEV), transform=tf, clips=clips).clone()
    assert lib.svt_debug_set(42, 0) == CLIPS_FAMILY + _form(precision, crop)
    b = m.forward_into(_host_batch(tf, roi, clips).to(DEV)).clone()
    assert lib.svt_debug_set(42, 0) // 100 * 100 == FLOAT_FAMILY
    assert torch.isfinite(a).all() and a.abs().max().item() > 0.1
    assert torch.equal(a, b)
    assert torch.equal(m.forward_into(roi.to(DEV)[..., None], transform=tf, clips=clips), a)      # the recipe's (B, T, H, W, 1) layout


def test_expected_kernels_of_the_cases_above():
    """88 and 60 select the 8-wide kernel in the 16-bit modes; so does 50 (see _form: the padded row is always a multiple of 8)."""
    for w in (88, 60, 50):
        assert _form("bf16", w) == _form("fp16", w) == WIDE_16
        assert _form("fp32", w) == _form("fp16x3", w) == GENERIC_F32


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["roi96", "roi97x99"])
def test_eval_plan_through_the_new_entry_equals_the_pinned_u8_entry(golden, name, precision):
    fx = golden("video_u8")[name]
    lib = _lib_of(precision)
    m = SubModel(512, fx["E"], "prelu", precision=precision, seed=1)
    m.load_state_dict(W.seeded_video_frontend_state_dict(fx["E"], seed=fx["weight_seed"]), strict=True)
    m = m.to(DEV)
    roi = torch.stack([fx["roi"], fx["roi"].flip(0)]).to(DEV)        # (2, T, H, W)
    T, H, Wd = roi.shape[1:]
    tf = EvalTransform()
    pinned = m.forward_into(roi).clone()
    assert lib.svt_debug_set(42, 0) == U8_FAMILY + _form(precision, 88)
    got = m.forward_into(roi, transform=tf, clips=tf.plan([T, T], H, Wd))
    assert lib.svt_debug_set(42, 0) == CLIPS_FAMILY + _form(precision, 88)
    assert torch.equal(got, pinned)


def test_a_batch_of_more_than_64_clips_is_split_over_launches():
    """65 one-frame clips of an 88 x 88 ROI, flips alternating from clip to clip: the last clip is alone in the second launch (the table
    in the kernel arguments holds 64).  Its padded operand and -- exact fp32 mode -- its features equal those of the clip forwarded
    alone; so do clip 63's (last of the first launch) and clip 0's."""
    m = _model("fp32")
    roi = _roi(65, 1, 88, 88, seed=65)
    clips = [VideoClip(0, 0, b % 2, 1) for b in range(65)]
    assert clips[64].flip != clips[63].flip
    tf = TrainTransform()
    y = m.forward_into(roi.to(DEV), transform=tf, clips=clips).clone()
    vp = _padded_operand(m, 65, 1, 88, 88).clone()
    for b in (64, 63, 0):
        one = m.forward_into(roi[b:b + 1].to(DEV), transform=tf, clips=[clips[b]]).clone()
        vp1 = _padded_operand(m, 1, 1, 88, 88)
        assert torch.equal(vp1[0].view(torch.int32), vp[b].view(torch.int32)), b
        want = torch.from_numpy(tf(roi[b].numpy(), draw=(0, 0, bool(clips[b].flip))))
        assert torch.equal(vp[b, 2:3, 3:91, 4:92].contiguous().view(torch.int32), want.view(torch.int32)), b
        assert torch.equal(one[0], y[b]), b


@pytest.mark.parametrize("field,bad,text", [
    ("dx", 99 - 88 + 1, "clip 1: dx = 12"),
    ("dy", -1, "clip 1: dy = -1"),
    ("flip", 2, "clip 1: flip = 2"),
    ("n_frames", 0, "clip 1: n_frames = 0"),
    ("n_frames", 6 + 1, "clip 1: n_frames = 7"),
])
def test_a_bad_clip_is_refused_before_anything_is_launched(field, bad, text):
    m = _model("fp32")
    roi = _roi(3, 6, 97, 99, seed=2).to(DEV)
    clips = list(THREE)
    clips[1] = clips[1]._replace(**{field: bad})
    fused = torch.full((3, 6, 2 * E), float("nan"), device=DEV)
    with pytest.raises(_lib.SvtError, match=text) as ei:
        m.forward_into(roi, fused, TrainTransform(), clips)
    assert "(status -1)" in str(ei.value)                                # SVT_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.isnan(fused).all(), "a refused call must not touch the output"
    good = m.forward_into(roi, fused, TrainTransform(), THREE)           # and the handle still works
    assert torch.isfinite(good[..., E:]).all() and not good[..., :E].any()


def test_clips_with_a_float_input_or_the_wrong_count_raise():
    m = _model("fp32")
    with pytest.raises(ValueError):
        m.forward_into(torch.zeros(3, 1, 6, 88, 88, device=DEV), clips=THREE)
    with pytest.raises(ValueError):
        m.forward_into(_roi(2, 6, 97, 99, seed=3).to(DEV), clips=THREE)


def test_video_probe_is_linear_probe_on_the_float_path_with_the_same_draws():
    """VideoProbe.fit_batch (uint8 clips, the draws made in the reference's order, transform + zero padding in the kernel) against
    LinearProbe.fit_features fed by the same frozen encoder on the host-transformed, zero-padded float frames of the same draws:
    head, loss terms and gradient norm equal after each of 3 steps; the draws are those of random.seed(7)."""
    from svt_speechbrain_amd.video import FairseqAVHubertPretrain
    cfg = S.PRESETS["tiny-avhubert-video"]
    enc = FairseqAVHubertPretrain(config=cfg, precision="fp32", seed=1, output_norm=True)
    enc.load_fairseq_model_state(W.seeded_avhubert_video_state_dict(cfg, seed=321))
    enc = enc.to(DEV)
    heads = []
    for _ in range(2):
        h = S.Linear(20, input_size=cfg.hidden_size)
        h.load_state_dict(W.seeded_head_state_dict(cfg.hidden_size, 20, seed=5))
        heads.append(h.to(DEV))
    probe = S.VideoProbe({"encoder": enc, "head": heads[0]}, lr=1.0)
    ref = S.LinearProbe({"encoder": enc, "head": heads[1]}, lr=1.0)
    g = torch.Generator().manual_seed(9)
    lengths = [12, 9]
    rois = [torch.randint(0, 256, (n, 96, 96), generator=g, dtype=torch.uint8) for n in lengths]
    anno = torch.stack([(torch.rand(2, 12, generator=g) < 0.5).float(), (torch.rand(2, 12, generator=g) < 0.5).float(),
                        torch.randint(0, 5, (2, 12), generator=g).float(), torch.randint(0, 13, (2, 12), generator=g).float()], -1).to(DEV)
    lens = torch.tensor([1.0, 9 / 12])
    padded = torch.zeros((2, 12, 96, 96), dtype=torch.uint8)
    padded[0], padded[1, :9] = rois[0], rois[1]
    tf = TrainTransform()
    replay = random.Random(7)
    random.seed(7)
    for step in range(3):
        want_clips = []
        for n in lengths:
            dx = replay.randint(0, 8)
            dy = replay.randint(0, 8)
            want_clips.append(VideoClip(dy, dx, int(replay.random() < 0.5), n))
        # a list of clips on even steps, the padded tensor with relative lengths on the odd one: the same batch
        if step % 2 == 0:
            loss = probe.fit_batch([r.to(DEV) for r in rois], lens, anno)
        else:
            loss = probe.fit_batch(padded.to(DEV), lens, anno)
        assert probe.last_clips == want_clips
        assert random.getstate() == replay.getstate()
        x = _host_batch(tf, padded, want_clips).to(DEV)
        loss_ref = ref.fit_features(enc({"video": x, "audio": None}), lens, anno)
        assert torch.isfinite(loss) and torch.equal(loss, loss_ref)
        assert probe.last_terms == ref.last_terms
        assert torch.equal(probe.last_grad_norm, ref.last_grad_norm)
        sa, sb = heads[0].state_dict(), heads[1].state_dict()
        assert sa.keys() == sb.keys()
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (step, k)
    assert not torch.equal(heads[0].state_dict()["w.weight"].cpu(), W.seeded_head_state_dict(cfg.hidden_size, 20, seed=5)["w.weight"])
    with pytest.raises(ValueError):
        probe.fit_batch(torch.zeros(2, 1, 12, 88, 88, device=DEV), lens, anno)
    with pytest.raises(_lib.SvtError):
        probe.fit_batch(padded, lens, anno)                              # on the CPU
