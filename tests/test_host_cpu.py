"""CPU tests (-m "not gpu"): host logic, state-dict schema, C-ABI symbol export, loud failure without a GPU."""
import ctypes
import os
import sys
import time
import re

import numpy as np
import pytest
import torch

import svt_speechbrain_amd as S
from svt_speechbrain_amd import _lib
from svt_speechbrain_amd import weights as W
from svt_speechbrain_amd.config import PRESETS, config_from_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    """Every function declared in include/svt_mi355.h is exported by the built .so and bound by _lib."""
    hdr = open(os.path.join(ROOT, "include", "svt_mi355.h")).read()
    declared = set(re.findall(r"\b(svt_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"svt_encoder_config"}
    assert declared == set(_lib.SYMBOLS.keys()), declared ^ set(_lib.SYMBOLS.keys())
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.svt_abi_version() == 1
    assert ctypes.sizeof(_lib.FrameC) == 16


def test_no_gpu_fails_loudly():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = _lib.load()
    assert lib.svt_device_count() == 0
    with pytest.raises(_lib.SvtError):
        _lib.require_gpu()
    enc = S.HuggingFaceWav2Vec2("tiny-group", None, config=PRESETS["tiny-group"])
    with pytest.raises(_lib.SvtError):
        enc(torch.zeros(1, 4000))
    with pytest.raises(_lib.SvtError):
        S.Linear(20, input_size=8)(torch.zeros(1, 8))
    with pytest.raises(_lib.SvtError):
        S.FusionRCA(d_model=64, nhead=8, d_ffn=128)(torch.zeros(1, 4, 64), torch.zeros(1, 4, 64))
    # C-ABI level: create on a machine without a device returns a status + message, never aborts
    cc = S.huggingface_interface._config_to_c(PRESETS["tiny-group"], True, True, "fp32")
    h = ctypes.c_void_p()
    rc = lib.svt_encoder_create(ctypes.byref(cc), 0, ctypes.byref(h))
    assert rc == -6 and b"no HIP device" in lib.svt_last_error()


def test_config_frames_and_flops():
    base = PRESETS["wav2vec2-base"]
    assert base.frames(160000) == 499 and base.frames(80000) == 249
    assert base.frame_counts(160000) == [31999, 15999, 7999, 3999, 1999, 999, 499]
    assert abs(base.flops_per_clip(160000) / 1e9 - 148.14) < 0.05
    assert abs(PRESETS["wav2vec2-large-lv60"].flops_per_clip(160000) / 1e9 - 383.86) < 0.1
    assert config_from_source("facebook/wav2vec2-base").hidden_size == 768
    assert config_from_source("facebook/wav2vec2-large-lv60").do_stable_layer_norm
    assert config_from_source("facebook/hubert-large-ll60k").family == "hubert"
    assert config_from_source("microsoft/wavlm-large").rel_pos_buckets == 320


def test_state_dict_schema_matches_hf_keys():
    for name in ["tiny-group", "tiny-layer", "tiny-hubert", "tiny-data2vec", "tiny-wavlm"]:
        cfg = PRESETS[name]
        enc = S.HuggingFaceWav2Vec2(name, None, config=cfg)
        keys = list(enc.state_dict().keys())
        assert keys == ["model." + k for k in W.encoder_param_shapes(cfg).keys()]
        for k, shp in W.encoder_param_shapes(cfg).items():
            assert tuple(enc.state_dict()["model." + k].shape) == shp
    assert not any(p.requires_grad for p in enc.parameters())  # freeze=True
    enc2 = S.HuggingFaceWav2Vec2("tiny-group", None, config=PRESETS["tiny-group"], freeze=False,
                                 freeze_feature_extractor=True)
    rg = {n: p.requires_grad for n, p in enc2.named_parameters()}
    assert not rg["model.feature_extractor.conv_layers.0.conv.weight"] and rg["model.encoder.layer_norm.weight"]
    lin = S.Linear(20, input_size=64)
    assert list(lin.state_dict().keys()) == ["w.weight", "w.bias"]
    fus = S.FusionRCA(d_model=64, nhead=8, d_ffn=128, max_length=50)
    assert list(fus.state_dict().keys())[0] == "fusion.positional_encoding.pe"
    assert fus.state_dict()["fusion.layer2.self_att.att.in_proj_weight"].shape == (192, 64)


def test_frame2note_matches_reference_golden(golden):
    for k, c in golden("frame2note").items():
        info = list(zip(c["p_on"].numpy(), c["p_off"].numpy(), c["oct"].tolist(), c["pc"].tolist()))
        assert S.frame2note(info, 0.4, 0.5, 1 / 49.8) == c["notes"], k
    with pytest.raises(ValueError):
        S.frame2note([(np.float32(0.9), np.float32(0.1), 1, 1)], 0.4, 0.5)
    assert S.frame2note([], 0.4, 0.5) == []


def test_filter_ctc_output_doctest():
    assert S.filter_ctc_output(['a', 'a', 'blank', 'b', 'b', 'blank', 'c'], blank_id='blank') == ['a', 'b', 'c']
    with pytest.raises(ValueError):
        S.filter_ctc_output("aab")


def test_shard_bounds_cover_and_order():
    from svt_speechbrain_amd.distributed import shard_bounds
    for n in [0, 1, 7, 32, 513]:
        for w in [1, 2, 3, 8]:
            spans = [shard_bounds(n, r, w) for r in range(w)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(spans[i][1] == spans[i + 1][0] for i in range(w - 1))
            assert max(h - l for l, h in spans) - min(h - l for l, h in spans) <= 1


def test_utterance_bounds_match_reference_rule():
    """MIR_ST500/prepare_benchmarks.py:117-126 + train_audio_ssl.py:373-390: round(duration/5) utterances, the last one
    takes the remainder (2.5 .. 7.5 s), bounds are round((i-1)*sr*5) .. round(i*sr*5)."""
    sr = 16000
    for dur in [5.0, 7.4, 7.6, 12.49, 12.51, 31.3, 2.6]:
        n = int(dur * sr)
        b = S.utterance_bounds(n, sr, 5.0)
        assert len(b) == max(1, round(n / sr / 5.0))
        assert b[0][0] == 0 and b[-1][1] == n
        assert all(b[i][1] == b[i + 1][0] for i in range(len(b) - 1))
        assert all(hi - lo == 5 * sr for lo, hi in b[:-1])
        if len(b) > 1 or n / sr >= 2.5:
            assert 0 < (b[-1][1] - b[-1][0]) / sr <= 7.5 + 1e-9
    assert S.feature_path("/x/song1") == "/x/song1/noise_data/clean_feats.pt"
    assert S.feature_path("/x/song1", True, "babble", -5) == "/x/song1/noise_data/babble/SNR_-5dB_feats.pt"


# ---- §8f rank 3: checkpoint directory reader ----
CKPT_TREE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ckpt_tree")


def test_checkpoint_selection_matches_reference_checkpointer():
    import json
    want = json.load(open(os.path.join(CKPT_TREE, "expected.json")))["picks"]
    ck = S.Checkpointer(CKPT_TREE)
    assert len(ck.list_checkpoints()) == 3
    assert ck.find_checkpoint().path.name == want["recent"]
    assert ck.find_checkpoint(min_key="loss").path.name == want["min_loss"]
    assert ck.find_checkpoint(max_key="COnPOff_f1").path.name == want["max_f1"]
    assert [c.path.name for c in ck.find_checkpoints(min_key="loss")] == want["ranked_min_loss"]
    assert [c.path.name for c in ck.find_checkpoints(max_key="COnPOff_f1")] == want["ranked_max_f1"]  # only those with the key
    assert [c.path.name for c in ck.find_checkpoints(min_key="loss", max_num_checkpoints=1)] == want["ranked_min_loss"][:1]
    with pytest.raises(ValueError):  # the reference's only conflict check: a key function together with a key name
        ck.find_checkpoints(importance_key=S.checkpoints.ckpt_recency, min_key="loss")
    assert S.Checkpointer(os.path.join(CKPT_TREE, "nowhere")).recover_if_possible() is None
    with pytest.raises(RuntimeError):  # a recoverable with no file in the checkpoint
        S.Checkpointer(CKPT_TREE, {"tokenizer": torch.nn.Linear(1, 1)}).recover_if_possible()
    S.Checkpointer(CKPT_TREE, {"tokenizer": torch.nn.Linear(1, 1)}, allow_partial_load=True).recover_if_possible()


def test_reference_checkpoint_files_load_unchanged_and_reproduce_the_reference_outputs():
    # the .ckpt files were written by the reference's Checkpointer around the reference's own modules; the package's
    # modules must take them as they are (HF key spelling, masked_spec_embed, w.weight / w.bias) — checked on the CPU
    # by running the oracle on the state the modules hold after loading
    import json
    from oracle import svt_oracle as O
    want = json.load(open(os.path.join(CKPT_TREE, "expected.json")))
    cfg = PRESETS["tiny-group"]
    enc = S.HuggingFaceWav2Vec2("tiny-group", None, config=cfg, seed=1)
    head = S.Linear(20, input_size=cfg.hidden_size)
    ck = S.Checkpointer(CKPT_TREE, {"wav2vec2": enc, "model": head})
    chosen = ck.recover_if_possible(min_key="loss")
    assert chosen.path.name == want["picks"]["min_loss"] and chosen.meta["loss"] == 0.47
    d = want["digests"][chosen.path.name]
    sd = {k[len("model."):]: v.detach().cpu() for k, v in enc.state_dict().items()}
    g = torch.Generator().manual_seed(d["wav_seed"])
    wav = (0.1 * torch.randn(2, 4000, generator=g)).clamp_(-1, 1)
    with torch.no_grad():
        logits = O.head_forward(O.encoder_forward(sd, cfg, wav), head.state_dict()["w.weight"].cpu(), head.state_dict()["w.bias"].cpu())
    assert abs(float(logits.double().sum()) - d["logits_sum"]) < 1e-3
    assert abs(float(logits.double().abs().sum()) - d["logits_abs"]) < 1e-3
    assert max(abs(float(a) - b) for a, b in zip(logits[0, 0, :4], d["first"])) < 2e-5


# ---- §8 a15: AV-HuBERT video encoder host side ----
def test_avhubert_video_state_dict_uses_fairseq_names_and_maps_onto_the_encoder():
    from svt_speechbrain_amd.video import FairseqAVHubertPretrain, SubModel
    from oracle import svt_oracle as O
    cfg = PRESETS["tiny-avhubert-video"]
    m = FairseqAVHubertPretrain(config=cfg, precision="fp32")
    keys = set(m.state_dict().keys())
    for k in ("model.feature_extractor_video.resnet.frontend3D.0.weight", "model.feature_extractor_video.resnet.trunk.layer4.1.bn2.running_var",
              "model.feature_extractor_video.proj.bias", "model.layer_norm.weight", "model.post_extract_proj.weight",
              "model.encoder.pos_conv.0.weight_g", "model.encoder.pos_conv.0.weight_v", "model.encoder.layers.1.self_attn.q_proj.weight",
              "model.encoder.layers.0.self_attn_layer_norm.bias", "model.encoder.layers.1.fc1.weight", "model.encoder.layers.1.fc2.bias",
              "model.encoder.layers.0.final_layer_norm.weight", "model.encoder.layer_norm.weight"):
        assert k in keys, k
    assert m.state_dict()["model.layer_norm.weight"].shape == (2 * cfg.hidden_size,)
    # every transformer key has an encoder slot, and the two key maps (package / oracle) agree and invert each other
    hf_keys = set(W.encoder_param_shapes(cfg, old_weight_norm_keys=True))
    seen = set()
    for k in keys:
        k = k[len("model."):]
        if k.startswith("feature_extractor_video."):
            continue
        hf = W.fairseq_to_hf_key(k)
        assert hf is not None and hf == O.fairseq_to_hf_key(k) and W.hf_to_fairseq_key(hf) == k
        seen.add(hf)
    assert seen == hf_keys
    # the front-end's keys are SubModel.state_dict()'s (139 entries in the reference, num_batches_tracked included)
    assert len(SubModel(512, 64, "prelu", precision="fp32").state_dict()) == 139
    with pytest.raises(_lib.SvtError):  # no GPU input -> loud failure, no CPU fallback
        m({"video": torch.zeros(1, 1, 2, 32, 32), "audio": None})


# ---- §8f rank 4: input pipeline and scoring (host code) ----
def test_batch_pad_right_and_padded_batch_match_reference_golden(golden):
    from svt_speechbrain_amd import dataio as D
    fx = golden("dataio")
    g = torch.Generator().manual_seed(31)
    for c in fx["pad"]:
        ts = [torch.randn(n, generator=g) for n in c["lens"]]
        data, valid = D.batch_pad_right(ts)
        assert tuple(data.shape) == c["shape"] and torch.equal(valid, c["valid"])
        assert abs(float(data.double().sum()) - c["checksum"]) < 1e-9
        if len(ts) > 1:
            assert bool((data[1, c["lens"][1]:] == 0).all())
    b = fx["batch"]
    pb = D.PaddedBatch(b["examples"])
    wavs, lens = pb.sig  # the unpacking compute_forward does
    assert torch.equal(wavs, b["sig"]) and torch.equal(lens, b["sig_lens"])
    assert torch.equal(pb.anno.data, b["anno"]) and torch.equal(pb.anno.lengths, b["anno_lens"])
    assert pb.id == b["ids"] and torch.equal(pb.cur_utter, b["cur"]) and len(pb) == 3
    assert pb["sig"].lengths is lens
    with pytest.raises(IndexError):
        D.batch_pad_right([])
    with pytest.raises(EnvironmentError):
        D.batch_pad_right([torch.zeros(3, 4), torch.zeros(2, 5)])


def test_manifest_slicing_rules(tmp_path):
    import csv
    from svt_speechbrain_amd import dataio as D
    # utterance plan of prepare_benchmarks.py:119-127 (round() is banker's rounding: 12.5 / 5 -> 2)
    assert D.plan_utterances(12.3) == [5, pytest.approx(7.3)]
    assert D.plan_utterances(7.4) == [7.4]
    assert D.plan_utterances(7.6) == [5, pytest.approx(2.6)]
    assert D.plan_utterances(12.5) == [5, 7.5]
    assert D.plan_utterances(27.49) == [5, 5, 5, 5, pytest.approx(7.49)]
    # the manifest as prepare_csv_benchmarks writes it
    p = tmp_path / "test.csv"
    with open(p, "w") as f:
        wr = csv.writer(f, delimiter=",", quotechar='"', quoting=csv.QUOTE_MINIMAL)
        wr.writerow(D.CSV_COLUMNS)
        for i, dur in enumerate(D.plan_utterances(12.3), start=1):
            wr.writerow([f"7_{i}", str(dur), "/data/7/vocals.wav", str(i), "2", "/data/7/frame_anno.npy", "/data/7/annotation.json"])
    rows = D.read_manifest(str(p))
    assert [r["ID"] for r in rows] == ["7_1", "7_2"] and rows[0]["duration"] == 5.0 and rows[1]["utter_num"] == "2"
    with open(p, "a") as f:
        f.write("7_2,1.0,a,1,1,b,c\n")
    with pytest.raises(ValueError):
        D.read_manifest(str(p))
    # slicing: the reference's expressions (train_audio_ssl.py:386-394, 412-420) evaluated literally
    sig = torch.arange(16000 * 12 + 4800, dtype=torch.float32)
    anno = torch.arange(612 * 4, dtype=torch.float32).view(612, 4)
    for uid, unum in [(1, 2), (2, 2), (1, 1), (2, 3), (3, 3)]:
        if uid == unum:
            want_s = sig[round((uid - 1) * 16000 * 5):]
            want_a = anno[round((uid - 1) * 49.8 * 5):]
        else:
            want_s = sig[round((uid - 1) * 16000 * 5):round(uid * 16000 * 5)]
            want_a = anno[round((uid - 1) * 49.8 * 5):round(uid * 49.8 * 5)]
        assert torch.equal(D.slice_audio(sig, str(uid), str(unum)), want_s)
        assert torch.equal(D.slice_annotation(anno, str(uid), str(unum)), want_a)
    assert D.slice_annotation(anno, 1, 2).shape[0] == 249 and D.slice_annotation(anno, 2, 3).shape[0] == 249  # round(249) .. round(498)


def test_mode_agreement_levels_and_near_ties():
    """svt_speechbrain_amd/agreement.py (what bench.py's parity leg and the 16-bit bounds of the GPU suite report), on hand-made logits:
    a flip across a 1e-5 margin is a near tie, a flip across a 1.0 margin is not; identical inputs agree at every level; the note
    metrics are micro-averaged over the clips."""
    from svt_speechbrain_amd.agreement import mode_agreement, note_agreement
    from svt_speechbrain_amd.decode import FRAME_DTYPE
    torch.manual_seed(0)
    ref = torch.randn(2, 60, 20)
    ref[..., 0] = -3.0
    ref[0, 10:14, 0] = 3.0; ref[0, 30, 1] = 3.0; ref[1, 5, 0] = 3.0          # a few onsets / an offset: notes exist
    ref[0, 3, 2], ref[0, 3, 3] = 5.0, 5.0 - 1e-5

    def frames(lg):
        fr = np.zeros(lg.shape[:2], dtype=FRAME_DTYPE)
        fr["p_on"], fr["p_off"] = torch.sigmoid(lg[..., 0]).numpy(), torch.sigmoid(lg[..., 1]).numpy()
        fr["octave"], fr["pitch_class"] = lg[..., 2:7].argmax(-1).numpy(), lg[..., 7:].argmax(-1).numpy()
        return fr

    same = mode_agreement(ref, frames(ref), ref, frames(ref))
    assert same["frames_argmax_mismatch"] == 0 and same["clips_with_identical_notes"] == 2 and same["COnPOff_f1"] == 1.0
    assert same["meets_1e-3_and_identical_notes"] and same["reference_notes"] > 0
    own = ref.clone()
    own[0, 3, 3] += 3e-5                                                       # breaks the near tie the other way
    r = mode_agreement(own, frames(own), ref, frames(ref))
    assert r["frames_argmax_mismatch"] == 1 and r["frames_argmax_mismatch_beyond_near_ties"] == 0 and r["max_abs_dlogit"] < 1e-3
    assert not r["meets_1e-3_and_identical_notes"] and r["meets_1e-3_and_identical_argmax_up_to_near_ties"]
    own[1, 7, 8] = ref[1, 7, 7:].max() + 1.0                                   # a hard flip of a pitch class
    r = mode_agreement(own, frames(own), ref, frames(ref))
    assert r["frames_argmax_mismatch"] == 2 and r["frames_argmax_mismatch_beyond_near_ties"] == 1
    assert not r["meets_1e-3_and_identical_argmax_up_to_near_ties"]
    # another head layout (3 octaves + 7 classes = 12 logits): the slices follow n_octave / n_class, not a hard-coded 13
    ref12 = torch.randn(1, 40, 12)
    ref12[0, 4, 5], ref12[0, 4, 6] = 6.0, 6.0 - 1e-5                          # classes 0 / 1 of the pitch-class slice (2 + 3 + ...)

    def frames12(lg):
        fr = np.zeros(lg.shape[:2], dtype=FRAME_DTYPE)
        fr["p_on"], fr["p_off"] = torch.sigmoid(lg[..., 0]).numpy(), torch.sigmoid(lg[..., 1]).numpy()
        fr["octave"], fr["pitch_class"] = lg[..., 2:5].argmax(-1).numpy(), lg[..., 5:].argmax(-1).numpy()
        return fr

    own12 = ref12.clone()
    own12[0, 4, 6] += 3e-5
    r = mode_agreement(own12, frames12(own12), ref12, frames12(ref12), n_octave=3, n_class=7)
    assert r["frames_argmax_mismatch"] == 1 and r["frames_argmax_mismatch_beyond_near_ties"] == 0
    with pytest.raises(ValueError):
        mode_agreement(own12, frames12(own12), ref12, frames12(ref12))        # 12 logits are not 2 + n_octave + 13
    # micro-average: 1 of 2 notes matched in one clip, 0 of 0 in the other -> precision 1/2, not the mean of (1/2, 1)
    na = note_agreement([[[0.0, 1.0, 60], [2.0, 3.0, 70]], []], [[[0.0, 1.0, 60], [2.5, 3.0, 64]], []])
    assert na["COnPOff_precision"] == 0.5 and na["COnPOff_recall"] == 0.5 and na["clips_with_identical_notes"] == 1


def test_transcription_scores_against_an_independent_maximum_matching():
    """scoring.py is PARITY UNPINNED (mir_eval absent), but every precision / recall / F number it returns depends only on the SIZE of a
    maximum bipartite matching of a hit graph whose rule is three comparisons -- and the size of a maximum matching is unique.  Here the
    hit graphs are rebuilt independently (plain loops over mir_eval's published rules) and matched by scipy's Hopcroft-Karp
    (scipy.sparse.csgraph.maximum_bipartite_matching, a third implementation): 300 random transcriptions with dense near-collisions."""
    import math
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_bipartite_matching
    from svt_speechbrain_amd import scoring as SC
    rng = np.random.default_rng(77)

    def size(hit):
        if hit.size == 0 or not hit.any():
            return 0
        return int((maximum_bipartite_matching(csr_matrix(hit.astype(np.int8)), perm_type="column") >= 0).sum())

    for trial in range(300):
        n_ref, n_est = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        # onsets on a 30 ms grid inside a short song: many notes within each other's 50 ms window; few distinct pitches; 10-cent detunings
        def notes(n):
            on = np.sort(rng.integers(0, 60, n) * 0.03 + rng.normal(0, 0.004, n).round(4)).clip(0, None)
            dur = rng.choice([0.06, 0.12, 0.3, 0.9], n)
            pitch = rng.choice([60, 60, 62, 64], n) + rng.choice([0.0, 0.1, 0.45, 0.55], n)
            return [[float(a), float(a + d), float(p)] for a, d, p in zip(on, dur, pitch)]
        ref, est = notes(n_ref), notes(n_est)
        on_hit = np.zeros((n_ref, n_est), bool); full = on_hit.copy(); nooff = on_hit.copy(); off_hit = on_hit.copy()
        for i, (ro, rf, rp) in enumerate(ref):
            for j, (eo, ef, ep) in enumerate(est):
                o = round(abs(ro - eo), 4) <= 0.05
                pch = abs(1200 * (math.log2(SC.midi_to_hz(rp)) - math.log2(SC.midi_to_hz(ep)))) <= 50.0
                f = round(abs(rf - ef), 4) <= max(0.2 * (rf - ro), 0.05)
                on_hit[i, j], nooff[i, j], full[i, j], off_hit[i, j] = o, o and pch, o and pch and f, f
        m = SC.score_song(est, ref)
        for key_p, key_r, hit in (("Precision", "Recall", full), ("Precision_no_offset", "Recall_no_offset", nooff),
                                  ("Onset_Precision", "Onset_Recall", on_hit), ("Offset_Precision", "Offset_Recall", off_hit)):
            k = size(hit)
            assert m[key_p] == pytest.approx(k / n_est) and m[key_r] == pytest.approx(k / n_ref), (trial, key_p, k)


def test_transcription_scores_hand_derived():
    # PARITY UNPINNED (mir_eval is not installed here): known answers derived by hand from mir_eval's published rules
    from svt_speechbrain_amd import scoring as SC
    ref = [[0.0, 1.0, 60], [1.0, 2.0, 62], [2.0, 3.0, 64]]
    est = [[0.02, 1.1, 60],      # onset, pitch, offset (0.1 <= max(0.2 * 1.0, 0.05)) all hit
           [1.06, 2.0, 62],      # onset 0.06 > 0.05: no hit at all
           [2.0, 3.5, 64.4],     # 40 cents ok, offset 0.5 > 0.2: counts only without the offset rule
           [5.0, 6.0, 70]]       # spurious
    m = SC.score_song(est, ref)
    assert m["Precision"] == pytest.approx(1 / 4) and m["Recall"] == pytest.approx(1 / 3) and m["F-measure"] == pytest.approx(2 / 7)
    assert m["Precision_no_offset"] == pytest.approx(2 / 4) and m["Recall_no_offset"] == pytest.approx(2 / 3)
    assert m["F-measure_no_offset"] == pytest.approx(4 / 7)
    assert m["Onset_Precision"] == pytest.approx(2 / 4) and m["Onset_Recall"] == pytest.approx(2 / 3)
    # pitch tolerance is in cents: 0.6 semitone off = 60 cents -> miss
    assert SC.score_song([[0.0, 1.0, 60.6]], [[0.0, 1.0, 60]])["F-measure_no_offset"] == 0.0
    # the boundary is inclusive after rounding to 4 decimals (0.05000001 -> hit)
    assert SC.score_song([[0.05000001, 1.0, 60]], [[0.0, 1.0, 60]])["Onset_F-measure"] == 1.0
    # maximum matching, not greedy: est X fits refs A and B, est Y fits A only -> both can be matched
    refs = [[1.00, 2.0, 60], [1.04, 2.0, 60]]
    ests = [[1.02, 2.0, 60], [0.96, 2.0, 60]]
    assert SC.score_song(ests, refs)["Onset_F-measure"] == 1.0 and SC.score_song(ests, refs)["F-measure"] == 1.0
    # empty sides score zero; malformed intervals raise
    assert SC.score_song([], refs)["F-measure"] == 0.0 and SC.score_song(ests, [])["Onset_Recall"] == 0.0
    with pytest.raises(ValueError):
        SC.score_song([[1.0, 1.0, 60]], refs)
    assert SC.midi_to_hz(69) == pytest.approx(440.0) and SC.midi_to_hz(57) == pytest.approx(220.0)
    # COff (N20EMv2/audio_only/train_audio_ssl.py:148-150): offsets alone, tolerance max(0.2 * ref duration, 0.05)
    #   est0 off 1.1 vs ref0 off 1.0 (tol 0.2) hit; est1 off 2.0 = ref1; est2 off 3.5 vs ref2 3.0 (tol 0.2) miss, but 3.5 is
    #   within no other ref; est3 off 6.0 none  -> 2 matches
    assert m["Offset_Precision"] == pytest.approx(2 / 4) and m["Offset_Recall"] == pytest.approx(2 / 3)
    assert m["Offset_F-measure"] == pytest.approx(4 / 7)
    # a long reference note widens its own offset window only: ref dur 2.0 -> tol 0.4
    assert SC.score_song([[0.0, 2.39, 60]], [[0.0, 2.0, 60]])["Offset_F-measure"] == 1.0
    assert SC.score_song([[0.0, 2.41, 60]], [[0.0, 2.0, 60]])["Offset_F-measure"] == 0.0
    assert SC.score_song([[0.5, 1.04, 60]], [[0.0, 1.0, 60]])["Offset_F-measure"] == 1.0   # floor of 50 ms
    # overlap ratio of the one fully matched pair: intersection [0.02, 1.0] / union [0.0, 1.1]
    assert m["Average_Overlap_Ratio"] == pytest.approx(0.98 / 1.1)
    assert m["Average_Overlap_Ratio_no_offset"] == pytest.approx((0.98 / 1.1 + 1.0 / 1.5) / 2)
    assert set(m) == {"Precision", "Recall", "F-measure", "Average_Overlap_Ratio", "Precision_no_offset", "Recall_no_offset",
                      "F-measure_no_offset", "Average_Overlap_Ratio_no_offset", "Onset_Precision", "Onset_Recall",
                      "Onset_F-measure", "Offset_Precision", "Offset_Recall", "Offset_F-measure"}


def test_config_from_source_family_heuristics():
    c = config_from_source
    assert c("facebook/wav2vec2-base").name == "wav2vec2-base" and c("facebook/wav2vec2-base-960h").hidden_size == 768
    assert c("facebook/wav2vec2-large-lv60").do_stable_layer_norm and c("facebook/wav2vec2-large-xlsr-53").feat_extract_norm == "layer"
    assert c("facebook/wav2vec2-large-960h").feat_extract_norm == "group" and not c("facebook/wav2vec2-large").do_stable_layer_norm
    assert c("facebook/hubert-large-ll60k").num_hidden_layers == 24 and c("facebook/hubert-base-ls960").num_hidden_layers == 12
    assert c("facebook/hubert-xlarge-ll60k").hidden_size == 1280
    assert c("ssl_model/AVHuBERT/large_vox_iter5.pt".replace("AVHuBERT", "avhubert")).family == "avhubert"
    assert c("facebook/data2vec-audio-base-960h").pos_conv_depth == 5 and c("facebook/data2vec-audio-large").hidden_size == 1024
    assert c("microsoft/wavlm-large").rel_pos_buckets == 320 and c("microsoft/wavlm-base-plus").num_hidden_layers == 12
    with pytest.raises(ValueError):
        c("my-model")
    # every preset's parameter schema is self-consistent (head_dim, group sizes)
    for name, cfg in PRESETS.items():
        assert cfg.hidden_size % cfg.num_attention_heads == 0 and cfg.hidden_size % cfg.num_conv_pos_embedding_groups == 0, name
        assert len(W.encoder_param_shapes(cfg)) > 0


@pytest.mark.parametrize("name", ["tiny-wav2vec2-hf", "tiny-hubert-bn-hf", "tiny-wavlm-hf", "tiny-data2vec-hf", "tiny-wav2vec2-sb"])
def test_local_model_directory_config_and_weights(golden, name, tmp_path):
    """Host side of the reference constructor's local-directory rules (huggingface_interface.py:215-262): config.json decides
    the geometry, preprocessor_config.json the waveform norm, *.bin = HuggingFace weights, *.ckpt = SpeechBrain-pretrained
    weights under "model.wav2vec2."; the parameter tree ends up with the reference model's keys and values."""
    import dataclasses
    import os
    fx = golden("local_ckpt")[name]
    d = os.path.join(os.path.dirname(__file__), "golden", "local_ckpt", name)
    enc = S.HuggingFaceWav2Vec2(d, str(tmp_path))
    want = dataclasses.asdict(PRESETS[fx["cfg"]])
    got = dataclasses.asdict(enc.config)
    for k in ("name", "family"):
        want.pop(k), got.pop(k)
    assert got == want
    assert enc.normalize_wav == fx["normalize_wav"]
    keys = [k for k in fx["keys"] if not k.endswith("masked_spec_embed")]
    assert sorted(enc.model.state_dict().keys()) == keys
    files = os.listdir(d)
    ck = [f for f in files if f.endswith(".bin") or f.endswith(".ckpt")][0]
    sd = torch.load(os.path.join(d, ck), map_location="cpu")
    pre = "model.wav2vec2." if ck.endswith(".ckpt") else ""
    for k, v in enc.model.state_dict().items():
        assert torch.equal(v, sd[pre + k]), k


def test_local_directory_without_checkpoint_raises_like_the_reference(tmp_path):
    import json
    (tmp_path / "config.json").write_text(json.dumps({"model_type": "wav2vec2"}))
    with pytest.raises(FileNotFoundError, match="does not contain a .bin or .ckpt checkpoint"):
        S.HuggingFaceWav2Vec2(str(tmp_path), str(tmp_path))


def test_frames2note_equals_the_frame_loop(golden):
    """The vectorised note assembly against the literal frame loop (itself pinned to the reference by the frame2note golden):
    the golden cases, random sequences with plateaus / exact-threshold values / pitch ties, and the edge lengths."""
    import time
    from svt_speechbrain_amd.decode import FRAME_DTYPE, frames2note

    def pack(p_on, p_off, octv, pc):
        fr = np.zeros(len(p_on), dtype=FRAME_DTYPE)
        fr["p_on"], fr["p_off"], fr["octave"], fr["pitch_class"] = p_on, p_off, octv, pc
        return fr

    for k, c in golden("frame2note").items():
        fr = pack(c["p_on"].numpy(), c["p_off"].numpy(), c["oct"].numpy(), c["pc"].numpy())
        assert frames2note(fr, 0.4, 0.5, 1 / 49.8) == c["notes"], k
    rng = np.random.default_rng(5)
    for trial in range(300):
        n = int(rng.integers(0, 400)) if trial else 9000
        # coarse grid of probabilities: many exact ties, values exactly on both thresholds
        grid = np.array([0.0, 0.1, 0.4, 0.5, 0.7, 0.7, 0.9, 1.0], dtype=np.float32)
        p_on = grid[rng.integers(0, len(grid), n)] * (rng.random(n) < 0.3)
        p_off = grid[rng.integers(0, len(grid), n)] * (rng.random(n) < 0.2)
        octv = rng.integers(0, 5, n)
        pc = rng.integers(0, 13, n)
        if trial % 3 == 0:  # long notes with few distinct pitches -> mode ties
            octv = np.repeat(rng.integers(0, 5, n // 7 + 1), 7)[:n]
            pc = np.repeat(rng.integers(0, 13, n // 3 + 1), 3)[:n]
        fr = pack(p_on.astype(np.float32), p_off.astype(np.float32), octv, pc)
        if n == 1 and p_on[0] >= np.float32(0.4):
            with pytest.raises(ValueError):
                frames2note(fr, 0.4, 0.5)
            continue
        t0 = time.time()
        want = S.frame2note(S.frames_to_info(fr), 0.4, 0.5, 1 / 49.8)
        t1 = time.time()
        got = frames2note(fr, 0.4, 0.5, 1 / 49.8)
        t2 = time.time()
        assert got == want, (trial, n)
        if n == 9000:
            print(f"9000 frames: loop {1e3 * (t1 - t0):.1f} ms, vectorised {1e3 * (t2 - t1):.1f} ms, {len(got)} notes")
    one = pack(np.float32([0.9]), np.float32([0.1]), [1], [1])
    with pytest.raises(ValueError):
        frames2note(one, 0.4, 0.5)
    assert frames2note(pack(np.float32([0.1]), np.float32([0.1]), [1], [1]), 0.4, 0.5) == []
    assert frames2note(pack([], [], [], []), 0.4, 0.5) == []


def test_frames2note_batch_c_routine_equals_the_frame_loop(golden):
    """svt_frames_to_notes (the library's host routine, one call per batch) against the literal frame loop: the reference's golden
    cases, random batches with plateaus / exact-threshold values / pitch ties (resolved by the reference's own expression), ragged
    lengths, and the reference's ValueError for a one-frame sequence above the onset threshold."""
    from svt_speechbrain_amd.decode import FRAME_DTYPE, frames2note_batch

    def pack(p_on, p_off, octv, pc):
        fr = np.zeros(len(p_on), dtype=FRAME_DTYPE)
        fr["p_on"], fr["p_off"], fr["octave"], fr["pitch_class"] = p_on, p_off, octv, pc
        return fr

    for k, c in golden("frame2note").items():
        fr = pack(c["p_on"].numpy(), c["p_off"].numpy(), c["oct"].numpy(), c["pc"].numpy())
        assert frames2note_batch(fr, 0.4, 0.5, 1 / 49.8) == [c["notes"]], k
    rng = np.random.default_rng(11)
    grid = np.array([0.0, 0.1, 0.4, 0.5, 0.7, 0.7, 0.9, 1.0], dtype=np.float32)
    ties = 0
    for trial in range(40):
        B, T = int(rng.integers(1, 9)), int(rng.integers(2, 600))
        fr = np.zeros((B, T), dtype=FRAME_DTYPE)
        fr["p_on"] = grid[rng.integers(0, len(grid), (B, T))] * (rng.random((B, T)) < 0.3)
        fr["p_off"] = grid[rng.integers(0, len(grid), (B, T))] * (rng.random((B, T)) < 0.2)
        if trial % 2:
            fr["octave"] = np.repeat(rng.integers(0, 5, (B, T // 7 + 1)), 7, axis=1)[:, :T]
            fr["pitch_class"] = np.repeat(rng.integers(0, 13, (B, T // 3 + 1)), 3, axis=1)[:, :T]
        else:
            fr["octave"] = rng.integers(0, 5, (B, T))
            fr["pitch_class"] = rng.integers(0, 13, (B, T))
        lengths = rng.integers(2, T + 1, B) if trial % 3 == 0 else None
        got = frames2note_batch(fr, 0.4, 0.5, 1 / 49.8, lengths=lengths)
        for b in range(B):
            n = T if lengths is None else int(lengths[b])
            want = S.frame2note(S.frames_to_info(fr[b, :n]), 0.4, 0.5, 1 / 49.8)
            assert got[b] == want, (trial, b)
            for note in want:
                lo_f, hi_f = round(note[0] * 49.8), round(note[1] * 49.8)
                seg = fr[b, lo_f:max(hi_f, lo_f + 1)]
                bag = [int(o) * 12 + int(p) for o, p in zip(seg["octave"], seg["pitch_class"]) if o != 4 and p != 12]
                ties += len(bag) > 0 and sorted(bag.count(v) for v in set(bag))[-2:].count(max(bag.count(v) for v in set(bag))) > 1
    assert ties > 20, "the random cases must exercise tied pitch histograms"
    one = pack(np.float32([0.9]), np.float32([0.1]), [1], [1])
    with pytest.raises(ValueError):
        frames2note_batch(one, 0.4, 0.5)
    assert frames2note_batch(pack(np.float32([0.1]), np.float32([0.1]), [1], [1]), 0.4, 0.5) == [[]]
    assert frames2note_batch(np.zeros((3, 0), dtype=FRAME_DTYPE), 0.4, 0.5) == [[], [], []]
    assert frames2note_batch(np.zeros((0, 5), dtype=FRAME_DTYPE), 0.4, 0.5) == []
    t0 = time.time()
    big = np.zeros((32, 499), dtype=FRAME_DTYPE)
    big["p_on"] = rng.random((32, 499)).astype(np.float32)
    big["p_off"] = rng.random((32, 499)).astype(np.float32)
    big["octave"] = rng.integers(0, 5, (32, 499))
    big["pitch_class"] = rng.integers(0, 13, (32, 499))
    for _ in range(10):
        frames2note_batch(big, 0.4, 0.5, 1 / 49.8)
    print(f"32 x 499 frames: {1e2 * (time.time() - t0):.2f} ms per batch")


def test_both_builds_of_the_library_export_the_cabi():
    """libsvt_mi355.so (bf16 operands) and libsvt_mi355_f16.so (IEEE-half operands, precision="fp16") export every symbol the header
    declares and say which one they are; the f16 build refuses the split-operand precision codes (they live in the bf16 build)."""
    a, b = _lib.load(), _lib.load("f16")
    assert a.svt_operand_type() == 0 and b.svt_operand_type() == 1 and a.svt_abi_version() == b.svt_abi_version() == 1
    for name in _lib.SYMBOLS:
        assert hasattr(a, name) and hasattr(b, name), name
    enc = S.HuggingFaceWav2Vec2("tiny-group", None, config=PRESETS["tiny-group"], precision="fp16", seed=1)
    assert enc._lib() is b
    with pytest.raises(ValueError):
        S.HuggingFaceWav2Vec2("tiny-group", None, config=PRESETS["tiny-group"], precision="fp8", seed=1)


def test_plain_c_caller_of_the_cabi_compiles(tmp_path):
    """tests/cabi/cabi_driver.c (C11, no torch, no Python) builds against include/svt_mi355.h with gcc; it runs in the GPU suite."""
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "cabi_driver")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(os.path.dirname(here), "include"), "-I", "/opt/rocm/include",
                        os.path.join(here, "cabi", "cabi_driver.c"), "-o", exe, "-L/opt/rocm/lib", "-lamdhip64", "-ldl",
                        "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert os.path.exists(exe)


def test_batched_gemm_descriptor_has_the_layout_the_header_declares(tmp_path):
    """svt_debug_gemm_desc as gcc lays it out from include/svt_mi355.h against _lib.GemmDescC: size and the offset of every field."""
    import subprocess
    fields = [f for f, _ in _lib.GemmDescC._fields_]
    src = tmp_path / "desc.c"
    src.write_text('#include <stdio.h>\n#include "svt_mi355.h"\nint main(void) {\n  printf("%zu", sizeof(svt_debug_gemm_desc));\n' +
                   "".join(f'  printf(" %zu", offsetof(svt_debug_gemm_desc, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = str(tmp_path / "desc")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.GemmDescC)] + [getattr(_lib.GemmDescC, f).offset for f in fields]
    hdr = open(os.path.join(ROOT, "include", "svt_mi355.h")).read()
    body = hdr[hdr.index("typedef struct svt_debug_gemm_desc {"):hdr.index("} svt_debug_gemm_desc;")]
    declared = re.findall(r"[\s,*](\w+)(?=[,;])", body)
    assert declared == fields, (declared, fields)


def test_layernorm_descriptor_has_the_layout_the_header_declares(tmp_path):
    """svt_debug_layernorm_desc as gcc lays it out from include/svt_mi355.h against _lib.LayerNormDescC: size and the offset of every field."""
    import subprocess
    fields = [f for f, _ in _lib.LayerNormDescC._fields_]
    src = tmp_path / "desc.c"
    src.write_text('#include <stdio.h>\n#include "svt_mi355.h"\nint main(void) {\n  printf("%zu", sizeof(svt_debug_layernorm_desc));\n' +
                   "".join(f'  printf(" %zu", offsetof(svt_debug_layernorm_desc, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = str(tmp_path / "desc")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.LayerNormDescC)] + [getattr(_lib.LayerNormDescC, f).offset for f in fields]
    hdr = open(os.path.join(ROOT, "include", "svt_mi355.h")).read()
    body = hdr[hdr.index("typedef struct svt_debug_layernorm_desc {"):hdr.index("} svt_debug_layernorm_desc;")]
    declared = re.findall(r"[\s,*](\w+)(?=[,;])", body)
    assert declared == fields, (declared, fields)


def test_conv0_descriptor_has_the_layout_the_header_declares(tmp_path):
    """svt_debug_conv0_desc as gcc lays it out from include/svt_mi355.h against _lib.Conv0DescC: size and the offset of every field."""
    import subprocess
    fields = [f for f, _ in _lib.Conv0DescC._fields_]
    src = tmp_path / "desc.c"
    src.write_text('#include <stdio.h>\n#include "svt_mi355.h"\nint main(void) {\n  printf("%zu", sizeof(svt_debug_conv0_desc));\n' +
                   "".join(f'  printf(" %zu", offsetof(svt_debug_conv0_desc, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = str(tmp_path / "desc")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.Conv0DescC)] + [getattr(_lib.Conv0DescC, f).offset for f in fields]
    hdr = open(os.path.join(ROOT, "include", "svt_mi355.h")).read()
    body = hdr[hdr.index("typedef struct svt_debug_conv0_desc {"):hdr.index("} svt_debug_conv0_desc;")]
    declared = re.findall(r"[\s,*](\w+)(?=[,;])", body)
    assert declared == fields, (declared, fields)


def test_video_step_descriptor_has_the_layout_the_header_declares(tmp_path):
    """svt_debug_video_desc as gcc lays it out from include/svt_mi355.h against _lib.VideoStepDescC: size and the offset of every field."""
    import subprocess
    fields = [f for f, _ in _lib.VideoStepDescC._fields_]
    src = tmp_path / "desc.c"
    src.write_text('#include <stdio.h>\n#include "svt_mi355.h"\nint main(void) {\n  printf("%zu", sizeof(svt_debug_video_desc));\n' +
                   "".join(f'  printf(" %zu", offsetof(svt_debug_video_desc, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = str(tmp_path / "desc")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.VideoStepDescC)] + [getattr(_lib.VideoStepDescC, f).offset for f in fields]
    hdr = open(os.path.join(ROOT, "include", "svt_mi355.h")).read()
    body = hdr[hdr.index("typedef struct svt_debug_video_desc {"):hdr.index("} svt_debug_video_desc;")]
    declared = re.findall(r"[\s,*](\w+)(?=[,;])", body)
    assert declared == fields, (declared, fields)


def test_encoder_step_descriptor_has_the_layout_the_header_declares(tmp_path):
    """svt_debug_encoder_desc as gcc lays it out from include/svt_mi355.h against _lib.EncoderStepDescC: size and the offset of every field."""
    import subprocess
    fields = [f for f, _ in _lib.EncoderStepDescC._fields_]
    src = tmp_path / "desc.c"
    src.write_text('#include <stdio.h>\n#include "svt_mi355.h"\nint main(void) {\n  printf("%zu", sizeof(svt_debug_encoder_desc));\n' +
                   "".join(f'  printf(" %zu", offsetof(svt_debug_encoder_desc, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = str(tmp_path / "desc")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.EncoderStepDescC)] + [getattr(_lib.EncoderStepDescC, f).offset for f in fields]
    hdr = open(os.path.join(ROOT, "include", "svt_mi355.h")).read()
    body = hdr[hdr.index("typedef struct svt_debug_encoder_desc {"):hdr.index("} svt_debug_encoder_desc;")]
    declared = re.findall(r"[\s,*](\w+)(?=[,;])", body)
    assert declared == fields, (declared, fields)


# ---- round-2 advisor findings: every way the weights can change must reach every device object ----
def test_state_loaded_through_a_parent_module_is_normalised_and_invalidates():
    """``Brain.modules`` is an ``nn.ModuleDict`` and ``Checkpointer`` may load through it: nn.Module recursion never calls
    the child's ``load_state_dict``, so the key normalisation (old weight-norm spelling, HF-only ``masked_spec_embed``) and
    the invalidation of the uploaded copy live in load hooks of ``.model``."""
    cfg = PRESETS["tiny-layer"]
    enc = S.HuggingFaceWav2Vec2("tiny-layer", None, config=cfg, seed=1)
    rep = enc.replica()
    parent = torch.nn.ModuleDict({"wav2vec2": enc, "model": S.Linear(20, input_size=cfg.hidden_size)})
    new = {"wav2vec2.model." + k: v for k, v in W.seeded_encoder_state_dict(cfg, seed=77, old_weight_norm_keys=True).items()}
    new["wav2vec2.model.masked_spec_embed"] = torch.zeros(cfg.hidden_size)
    new.update({"model." + k: v for k, v in parent["model"].state_dict().items()})
    g0 = enc._gen[0]
    res = parent.load_state_dict(new, strict=True)          # strict: the reference's checkpoint hook (utils/checkpoints.py:69-95)
    assert not res.missing_keys and not res.unexpected_keys
    assert enc._gen[0] > g0 and rep._gen is enc._gen        # the replica sees the same generation counter
    want = W.seeded_encoder_state_dict(cfg, seed=77)
    for k, v in enc.model.state_dict().items():
        assert torch.equal(v, want[k]), k
    g1 = enc._gen[0]
    enc.model.load_state_dict(want, strict=True)             # loading straight into .model invalidates too
    assert enc._gen[0] > g1
    g2 = enc._gen[0]
    rep.load_state_dict({"model." + k: v for k, v in want.items()})   # ... and so does loading into a replica
    assert enc._gen[0] > g2
    g3 = enc._gen[0]
    enc.refresh()
    assert enc._gen[0] > g3


def test_replica_and_data_parallel_replica_device_state():
    """``replica()``: same parameters, OWN registry of device objects.  ``nn.DataParallel`` replicas (``replicate`` shallow-copies
    ``__dict__``) SHARE the registry, so nothing is freed twice and each device keeps one C object across forwards."""
    cfg = PRESETS["tiny-group"]
    enc = S.HuggingFaceWav2Vec2("tiny-group", None, config=cfg)
    rep = enc.replica()
    assert rep._dev is not enc._dev and rep.model is enc.model
    dp = enc._replicate_for_data_parallel()
    assert dp._dev is enc._dev and dp._gen is enc._gen and dp._dp_replica and not enc._dp_replica
    for mod in (S.Linear(20, input_size=64), S.FusionRCA(d_model=64, nhead=8, d_ffn=128, max_length=50)):
        r = mod._replicate_for_data_parallel()
        assert r._dev is mod._dev
    from svt_speechbrain_amd._device import DeviceObjects
    d = DeviceObjects("svt_encoder_destroy")
    a = d.slot(0, ("x",))
    assert d.slot(0, ("x",)) is a and d.slot(1, ("x",)) is not a
    assert d.slot(0, ("y",)) is not a        # other flags on the same device: the old slot is replaced
    d.close()


def simulated_replicate(net):
    """What ``torch.nn.parallel.replicate`` does to a module tree, without devices: every module is shallow-copied by its own
    ``_replicate_for_data_parallel`` (which empties ``_parameters``), children are re-linked to the copies, and the broadcast
    parameter copies (here: clones) become PLAIN attributes -- so ``parameters()`` / ``state_dict()`` of a replica hold no weights."""
    mods = list(net.modules())
    idx = {id(m): i for i, m in enumerate(mods)}
    copies = [m._replicate_for_data_parallel() for m in mods]
    for m, r in zip(mods, copies):
        for k, child in m._modules.items():
            r._modules[k] = None if child is None else copies[idx[id(child)]]
        for k, p_ in m._parameters.items():
            if p_ is not None:
                setattr(r, k, p_.detach().clone())
    return copies[0]


def test_data_parallel_replica_uploads_the_original_parameters():
    """A REAL replica has no parameters of its own (``replicate`` hangs per-forward copies on it as plain attributes): the upload
    loop and the change signature of a replica must walk the module it was replicated from."""
    cfg = PRESETS["tiny-group"]
    enc = S.HuggingFaceWav2Vec2("tiny-group", None, config=cfg)
    rep = simulated_replicate(enc)
    assert rep is not enc and rep._param_owner() is enc and "_dp_origin" not in rep._modules
    assert len(list(rep.model.parameters())) == 0          # the trap: nothing to upload from the replica's own tree
    own = {k for k, v in enc.model.state_dict().items() if v.is_floating_point()}
    got = dict(rep._param_owner()._upload_items())
    assert set(got) == own and len(own) > 20
    assert rep._param_owner()._sentinel() == enc._sentinel()
    # a replica of a replica (nested DataParallel) still points at the original
    assert simulated_replicate(rep)._param_owner() is enc
    head = S.Linear(20, input_size=64)
    hr = simulated_replicate(head)
    w, b = hr._param_owner()._upload_items()
    assert w is head.w.weight and b is head.w.bias and hr._devs is head._devs
    fus = S.FusionRCA(d_model=64, nhead=8, d_ffn=128, max_length=50)
    fr = simulated_replicate(fus)
    assert len(list(fr.fusion.parameters())) == 0
    assert [n for n, _ in fr._param_owner()._tensors()] == [n for n, _ in fus._tensors()] and len(list(fus._tensors())) > 10
    from svt_speechbrain_amd.video import SubModel
    sm = SubModel(embed_dim=32)
    sr = simulated_replicate(sm)
    assert [n for n, _ in sr._param_owner()._tensors()] == [n for n, _ in sm._tensors()]


def test_amt_forward_accepts_both_recipes_module_names():
    """The audio-visual recipe names its modules ``fusion`` + ``head`` (train_rca_av.py:39,44 / its yaml ``modules:``), the
    audio-only ones ``wav2vec2`` + ``model`` (train_audio_ssl.py:36-39)."""
    calls = []

    class M:
        def __init__(self, tag): self.tag = tag
        def __call__(self, *a):
            calls.append(self.tag)
            return torch.zeros(2, 5, 20) if self.tag != "fusion" else torch.zeros(2, 5, 8)
    amt = S.AMTForward({"fusion": M("fusion"), "head": M("head")})
    out = amt.compute_forward(torch.zeros(2, 5, 8), torch.ones(2), videos=torch.zeros(2, 5, 8))
    assert calls == ["fusion", "head"] and len(out) == 5 and out[2].shape == (2, 5, 5) and out[3].shape == (2, 5, 13)
    calls.clear()
    S.AMTForward({"fusion": M("fusion"), "model": M("model")}).compute_forward(torch.zeros(2, 5, 8), None, videos=torch.zeros(2, 5, 8))
    assert calls == ["fusion", "model"]
    with pytest.raises(KeyError):
        S.AMTForward({"fusion": M("fusion")}).compute_forward(torch.zeros(2, 5, 8), None, videos=torch.zeros(2, 5, 8))
    # the fused tail re-associates the out-norm and the head: default only in the throughput precisions
    assert S.AMTForward({}).fuse_tail is None


def test_bench_refuses_a_rank_count_mismatch_and_lib_variant_path():
    import subprocess, sys
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29999")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], env=env,
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "--gpus 2" in (r.stderr + r.stdout), (r.stdout[-500:], r.stderr[-500:])
    # the IEEE-half build's file name is derived from the SUFFIX of the library path only
    root, ext = os.path.splitext(_lib.LIB_PATH)
    assert ext == ".so" and os.path.exists(f"{root}_f16{ext}")


def test_bench_help_lists_full_and_the_legs_it_gates():
    """`bench.py --help` prints (every help string formats) and names --full, off by default, as what the skip flags qualify."""
    import subprocess, sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = " ".join(r.stdout.split())
    assert "--full" in out and "(off by default)" in out
    for flag in ("--no-cpu-baseline", "--no-extra-legs", "--no-parity-leg"):
        assert f"{flag} with --full:" in out, flag


def test_local_directory_picks_the_weights_file_and_reads_shards(tmp_path):
    """A Trainer output directory holds optimizer.bin / training_args.bin beside the weights, and large checkpoints come as
    shards with an index: the wrapper must load pytorch_model.bin (or the shards), never the alphabetically first *.bin."""
    import json
    cfg = PRESETS["tiny-group"]
    sd = W.seeded_encoder_state_dict(cfg, seed=5)
    (tmp_path / "config.json").write_text(json.dumps({
        "model_type": "wav2vec2", "hidden_size": 64, "num_hidden_layers": 2, "num_attention_heads": 4, "intermediate_size": 128,
        "conv_dim": [32] * 7, "num_conv_pos_embeddings": 16, "num_conv_pos_embedding_groups": 4}))
    (tmp_path / "preprocessor_config.json").write_text(json.dumps({"do_normalize": False}))
    torch.save({"state": torch.zeros(3)}, tmp_path / "optimizer.bin")
    torch.save({"lr": 1.0}, tmp_path / "a_training_args.bin")
    torch.save(sd, tmp_path / "pytorch_model.bin")
    enc = S.HuggingFaceWav2Vec2(str(tmp_path), str(tmp_path))
    assert enc.normalize_wav is False
    for k, v in enc.model.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # sharded form
    (tmp_path / "pytorch_model.bin").unlink()
    keys = list(sd.keys())
    half = len(keys) // 2
    torch.save({k: sd[k] for k in keys[:half]}, tmp_path / "pytorch_model-00001-of-00002.bin")
    torch.save({k: sd[k] for k in keys[half:]}, tmp_path / "pytorch_model-00002-of-00002.bin")
    wm = {k: ("pytorch_model-00001-of-00002.bin" if i < half else "pytorch_model-00002-of-00002.bin") for i, k in enumerate(keys)}
    (tmp_path / "pytorch_model.bin.index.json").write_text(json.dumps({"weight_map": wm}))
    enc2 = S.HuggingFaceWav2Vec2(str(tmp_path), str(tmp_path))
    for k, v in enc2.model.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_pretrain_without_weights_and_do_normalize_defaults(caplog):
    from svt_speechbrain_amd.config import preset_do_normalize
    with pytest.raises(FileNotFoundError, match="no local checkpoint"):
        S.HuggingFaceWav2Vec2("facebook/wav2vec2-base", None, allow_random_init=False)
    with caplog.at_level("WARNING"):
        enc = S.HuggingFaceWav2Vec2("facebook/wav2vec2-base", None)     # the recipes' call: weights come from the Checkpointer later
    assert "SEEDED RANDOM" in caplog.text
    assert enc.normalize_wav is True
    # the reference reads feature_extractor.do_normalize: False for the LibriSpeech-960 BASE models of HuBERT / WavLM
    assert preset_do_normalize("facebook/hubert-base-ls960") is False and preset_do_normalize("microsoft/wavlm-base") is False
    assert preset_do_normalize("facebook/hubert-large-ll60k") is True and preset_do_normalize("some/unknown-model") is None
    assert S.HuggingFaceWav2Vec2("facebook/hubert-base-ls960", None, pretrain=False).normalize_wav is False
    assert S.HuggingFaceWav2Vec2("facebook/hubert-base-ls960", None, pretrain=False, normalize_wav=True).normalize_wav is True


def test_operand_rounding_simulation_brackets_the_exact_oracle():
    """tools/sim_split.py (the yardstick of the 16-bit modes' bounds in tests/test_gpu_parity.py): rounding every dense product's operands to
    bf16 costs about ten times what rounding them to IEEE half costs, the three-product split reproduces the golden to 1e-3 / 1e-4, and no
    argmax moves on the tiny golden."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sim_split
    fx = torch.load(os.path.join(ROOT, "tests", "golden", "tiny_group.pt"), weights_only=False)
    b1 = sim_split.simulate(fx, "bf16x1")
    h1 = sim_split.simulate(fx, "f16x1")
    b3 = sim_split.simulate(fx, "bf16x3")
    h3 = sim_split.simulate(fx, "f16x3")
    assert 0.02 < b1[0] < 0.3 and b1[0] > 4 * h1[0]
    assert b3[0] < 1e-3 and h3[0] < 1e-4
    assert b1[2] == h1[2] == b3[2] == h3[2] == 0 and b1[3] == fx["logits"].shape[0] * fx["logits"].shape[1]


def test_committed_simulation_bounds_are_what_the_simulation_gives():
    """tests/golden/sim_bounds.json (the yardstick the GPU suite holds the 16-bit modes to) against a fresh run of tools/sim_split.py on
    the cases that take seconds here; every bound case of the GPU suite must be in the table."""
    import json
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sim_split
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "sim_bounds.json")))
    # the table is only as good as the sources it was computed from: a change of the oracle or of the simulation without a re-run
    # of tests/golden/make_sim_bounds.py fails here (the large cases are not re-derived below)
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_sim_bounds
    assert table["_sources_sha256"] == make_sim_bounds.source_digest(), \
        "oracle/svt_oracle.py or tools/sim_split.py changed: re-run python tests/golden/make_sim_bounds.py and commit sim_bounds.json"
    for name in ("tiny_group", "tiny_layer", "base_c1", "base_b2", "large_c1", "data2vec_base_c1", "wavlm_base_c1", "large_b2", "hubert_large_b2"):
        assert set(table[name]) == {"bf16x1", "f16x1", "bf16x1s", "f16x1s"} and all(len(v) == 8 for v in table[name].values())
    torch.set_num_threads(8)
    for name in ("tiny_group", "tiny_layer", "base_c1"):
        fx = torch.load(os.path.join(ROOT, "tests", "golden", f"{name}.pt"), weights_only=False)
        for mode in ("bf16x1", "f16x1", "bf16x1s", "f16x1s"):
            mx, mean, mism, frames, n_ref, f_full, f_nooff, f_on = sim_split.simulate(fx, mode)
            t = table[name][mode]
            assert n_ref == t[4] and abs(f_full - t[5]) <= 2.0 / max(1, n_ref) and abs(f_on - t[7]) <= 2.0 / max(1, n_ref), (name, mode)
            # another BLAS thread count may move the last bits of a sum, hence a near-tie frame
            assert abs(mx - t[0]) <= 0.02 * t[0] + 1e-5 and abs(mean - t[1]) <= 0.01 * t[1] + 1e-6 and abs(mism - t[2]) <= 1 and frames == t[3], (name, mode)


def test_bench_dump_outputs_writes_float_arrays_and_samples_beyond_the_limit(tmp_path):
    """bench.py --dump-outputs: frames split into their four fields (the float fields keep their bits), every file float32 / float64,
    and above the size limit the same seeded sample of clips in every array, its indices beside them."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("svt_bench_module", os.path.join(ROOT, "bench.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    n, T = 6, 5
    p_on = torch.rand(n, T)
    words = torch.stack([p_on.view(torch.int32), (1 - p_on).view(torch.int32), torch.randint(0, 5, (n, T), dtype=torch.int32),
                         torch.randint(0, 13, (n, T), dtype=torch.int32)], -1)
    f = B.frame_fields(words, T)
    assert np.array_equal(f["frame_p_on"], p_on.numpy()) and f["frame_p_on"].dtype == np.float32
    assert np.array_equal(f["frame_octave"], words[..., 2].numpy()) and f["frame_octave"].dtype == np.float64
    arrays = dict(f, logits=torch.randn(n, T, 20).numpy())
    names = B.dump_outputs(str(tmp_path / "all"), arrays)
    assert names == sorted(arrays)
    for k in names:
        a = np.load(tmp_path / "all" / f"{k}.npy")
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, arrays[k])
    per_clip = sum(a.nbytes for a in arrays.values()) // n
    limit = 3 * per_clip + 100
    names = B.dump_outputs(str(tmp_path / "part"), arrays, limit=limit)
    assert "clip_index" in names
    idx = np.load(tmp_path / "part" / "clip_index.npy")
    assert len(idx) == 3 and np.all(np.diff(idx) > 0)
    assert sum(os.path.getsize(tmp_path / "part" / f"{k}.npy") - 128 for k in names) <= limit
    assert np.array_equal(np.load(tmp_path / "part" / "logits.npy"), arrays["logits"][idx.astype(int)])
    B.dump_outputs(str(tmp_path / "again"), arrays, limit=limit)
    assert np.array_equal(np.load(tmp_path / "again" / "clip_index.npy"), idx)
