"""Generate tests/golden/resample.pt by running the REFERENCE's own speechbrain/processing/speech_augmentation.py, unmodified.

Runs only where the reference checkout is present (REF below); the fixture it writes holds data only -- tables, seeds, digests, outputs --
and the reference itself is never committed.

    python tests/golden/make_golden_resample.py

speech_augmentation.py is loaded by file path; the three speechbrain modules it imports at the top (dataio.legacy, dataio.dataloader,
processing.signal_processing: data loading and the noise / reverb helpers, none of which Resample touches) are permissive stubs.  For each
ratio of tests/resample_limit.py RATIOS the fixture records

    first_indices, weights        Resample._indices_and_weights (fp32, on the CPU)
    P, S, W
    n_out                         Resample._output_samples for input lengths 1 .. 2000 (int16)
    cases[n]                      for n in LENGTHS: the seed and sha256 of the (2, n) input (tests/resample_limit.py seeded_input), the
                                  reference's forward of it as [batch = 2, time], and ref_vs_fp64 = the largest
                                  |reference - fp64 sum| / limit over both rows (tests/resample_limit.py: exact, limit)"""
import importlib.util
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import resample_limit as RL  # noqa: E402

REF = "/root/reference"


class Stub(types.ModuleType):
    __path__ = []

    def __getattr__(self, n):
        if n.startswith("__"):
            raise AttributeError(n)
        return Stub(self.__name__ + "." + n)

    def __call__(self, *a, **k):
        return None


def main():
    for m in ["speechbrain", "speechbrain.dataio", "speechbrain.dataio.legacy", "speechbrain.dataio.dataloader", "speechbrain.processing",
              "speechbrain.processing.signal_processing"]:
        sys.modules.setdefault(m, Stub(m))
    spec = importlib.util.spec_from_file_location("ref_speech_augmentation", REF + "/speechbrain/processing/speech_augmentation.py")
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    fx = {"ratios": list(RL.RATIOS), "lengths": list(RL.LENGTHS), "tables": {}}
    for orig, new in RL.RATIOS:
        rs = ref.Resample(orig_freq=orig, new_freq=new)
        rec = {"S": rs.conv_stride, "P": rs.conv_transpose_stride, "cases": {}}
        for n in RL.LENGTHS:
            seed = RL.input_seed(orig, new, n)
            x = RL.seeded_input(2, n, seed)
            with torch.no_grad():
                y = rs(x)
            first, weights = rs.first_indices.to(torch.int32), rs.weights
            assert y.shape == (2, rs._output_samples(n)) and y.dtype == torch.float32
            want, M = RL.exact(x, first, weights, rs.conv_stride, y.shape[1])
            rec["cases"][n] = {"seed": seed, "sha256": RL.sha256(x), "out": y.clone(),
                               "ref_vs_fp64": RL.worst(y, want, RL.limit(M, weights.shape[1]))}
        assert torch.equal(rs.first_indices, rs.first_indices.to(torch.int32).float())
        rec["first_indices"], rec["weights"], rec["W"] = rs.first_indices.to(torch.int32), rs.weights.clone(), rs.weights.shape[1]
        rec["n_out"] = torch.tensor([rs._output_samples(n) for n in range(1, RL.N_OUT_LENGTHS + 1)], dtype=torch.int16)
        fx["tables"][orig, new] = rec
        print(f"{orig} -> {new}: P {rec['P']} S {rec['S']} W {rec['W']} first {int(rec['first_indices'].min())} .. "
              f"{int(rec['first_indices'].max())}; ref_vs_fp64 " + ", ".join(f"{n}: {c['ref_vs_fp64']:.3f}" for n, c in rec["cases"].items()))
    out = os.path.join(HERE, "resample.pt")
    torch.save(fx, out)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
