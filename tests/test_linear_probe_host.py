"""Host-side checks of the linear-probe step (no GPU): the reference fixture's trajectory replays in plain torch on the CPU, the optimizer
keeps torch's Adadelta interface, and the GPU-only pieces refuse CPU tensors loudly."""
import hashlib

import pytest
import torch

import svt_speechbrain_amd as S
from svt_speechbrain_amd import _lib
from svt_speechbrain_amd import training as TR
from svt_speechbrain_amd import weights as W


def fixture_inputs(fx):
    """The waveform and the initial head of tests/golden/linear_probe.pt, rebuilt from their seeds (the fixture keeps digests)."""
    g = torch.Generator().manual_seed(fx["wav_seed"])
    wav = (0.1 * torch.randn(fx["B"], fx["L"], generator=g)).clamp_(-1, 1)
    wav[1, fx["pad_from"]:] = 0.0
    head = W.seeded_head_state_dict(fx["feats"].shape[-1], 20, seed=fx["head_seed"])
    return wav, head


def sd_digest(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().contiguous().numpy().tobytes())
    return h.hexdigest()


def sampled(t, idx):
    """A weight cut down to the entries the fixture records (flattened, at idx); a bias whole."""
    return t.detach().cpu().reshape(-1)[idx.long()] if t.dim() == 2 else t.detach().cpu()


def _objective(logits, anno, wav_lens, pw):
    """compute_objectives (MIR_ST500/train_audio_ssl.py:50-76) with compute_masked_loss / truncate semantics, plain torch."""
    T = min(logits.shape[1], anno.shape[1])
    x, a = logits[:, :T], anno[:, :T]
    m = (torch.arange(T, dtype=torch.float32)[None, :] < (wav_lens * T)[:, None]).float()
    f = torch.nn.functional
    on = (f.binary_cross_entropy_with_logits(x[:, :, 0], a[:, :, 0], pos_weight=torch.tensor([pw]), reduction="none") * m).sum() / m.sum()
    off = (f.binary_cross_entropy_with_logits(x[:, :, 1], a[:, :, 1], reduction="none") * m).sum() / m.sum()
    octv = (f.nll_loss(torch.log_softmax(x[:, :, 2:7], -1).transpose(1, 2), a[:, :, 2].long(), reduction="none") * m).sum() / m.sum()
    cls = (f.nll_loss(torch.log_softmax(x[:, :, 7:], -1).transpose(1, 2), a[:, :, 3].long(), reduction="none") * m).sum() / m.sum()
    return [on, off, octv, cls]


@pytest.mark.parametrize("case", ["lr1", "lr3e-4"])
def test_reference_fixture_replays_in_plain_torch(golden, case):
    fx = golden("linear_probe")
    c = fx["cases"][case]
    feats, lens = fx["feats"], fx["wav_lens"]
    assert fx["T"] == feats.shape[1] and 1 <= abs(c["anno"].shape[1] - fx["T"]) <= 3 and float(lens.min()) < 1
    assert (c["anno"][:, :, 2] == -100).any()
    wav, hd = fixture_inputs(fx)
    assert hashlib.sha256(wav.numpy().tobytes()).hexdigest() == fx["wav_sha256"] and sd_digest(hd) == fx["head_sha256"]
    idx = fx["sampled_index"]
    lin = torch.nn.Linear(feats.shape[-1], 20)
    lin.load_state_dict({"weight": hd["w.weight"], "bias": hd["w.bias"]})
    opt = torch.optim.Adadelta(lin.parameters(), lr=c["lr"], rho=fx["rho"], eps=fx["eps"])
    for step in range(len(c["params"])):
        terms = _objective(lin(feats), c["anno"], lens, fx["onset_positive_weight"])
        loss = sum(terms)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(lin.parameters(), fx["max_grad_norm"])
        opt.step()
        opt.zero_grad()
        got = torch.tensor([float(t.detach()) for t in terms])
        assert torch.allclose(got, c["terms"][step][:4], rtol=1e-5, atol=0), (step, got, c["terms"][step])
        assert torch.allclose(sampled(lin.weight, idx), c["params"][step]["w.weight"], rtol=0, atol=1e-6)
        assert torch.allclose(lin.bias.detach(), c["params"][step]["w.bias"], rtol=0, atol=1e-6)
    assert c["grad_norms"][0] > fx["max_grad_norm"]   # the clip is exercised


def test_adadelta_keeps_torch_interface():
    p = torch.nn.Parameter(torch.zeros(3))
    ours, theirs = TR.Adadelta([p], lr=0.5, rho=0.95, eps=1e-8), torch.optim.Adadelta([p], lr=0.5, rho=0.95, eps=1e-8)
    assert ours.defaults == theirs.defaults
    assert ours.state_dict()["param_groups"] == theirs.state_dict()["param_groups"]
    for bad in (dict(lr=-1.0), dict(rho=1.5), dict(eps=-1.0), dict(weight_decay=-0.1)):
        with pytest.raises(ValueError):
            TR.Adadelta([p], **bad)
    assert S.Adadelta is TR.Adadelta and S.LinearProbe is TR.LinearProbe


def test_gpu_only_pieces_refuse_cpu_tensors():
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(_lib.SvtError, match="no CPU fallback"):
        TR.Adadelta([p]).step()
    assert torch.equal(p.detach(), torch.zeros(4))
    with pytest.raises(_lib.SvtError):
        TR.amt_objective_grad(torch.zeros(1, 4, 20), *(torch.zeros(1, 4),) * 4)
    with pytest.raises(_lib.SvtError):
        TR.linear_backward(torch.zeros(4, 8), torch.zeros(4, 2))


def test_linear_probe_takes_the_recipe_modules_and_needs_the_fused_optimizer():
    head = S.Linear(20, input_size=64)
    probe = S.LinearProbe({"wav2vec2": None, "model": head})
    assert probe.head is head and probe.max_grad_norm == 5.0 and probe.nonfinite_patience == 3
    assert probe.optimizer.defaults["lr"] == 3e-4 and probe.optimizer.defaults["rho"] == 0.95
    with pytest.raises(TypeError):
        S.LinearProbe({"wav2vec2": None, "model": head}, optimizer=torch.optim.Adadelta(head.parameters()))
    with pytest.raises(_lib.SvtError):
        probe.fit_features(torch.zeros(1, 5, 64), None, torch.zeros(1, 5, 4))
