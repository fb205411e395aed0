#!/usr/bin/env python3
"""Generate tests/golden/mixed_modal.npz: the reference's MVAE.forward (vae.py:126-165) in eval() mode on the seeded batch of
tests/avail_cases.py, the WHOLE batch once per modality subset (the seven subsets of {visual, tactile, pose}), one injected eps
for the batch.  Row b of the fixture is row b of the run of row b's subset: what a mixed-modality batch must reproduce in one
request.  Two models: the unconditional cnn-mvae + pose ("plain") and the categorical-condition one ("cat").  Results only: the
inputs are regenerated from their seeds.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_mixed.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as G  # noqa: E402
import avail_cases as A  # noqa: E402

import torch  # noqa: E402

from mmdyn_hip.utils.seeded_init import seeded_state_dict, seeded_running_stats  # noqa: E402


def gen(tag, categorical, out):
    inputs, eps, cond = A.case(categorical)
    kw = A.model_kw(categorical)
    model = G.M.setup_model("cnn-mvae", cross_modal=True, **kw)
    model.load_state_dict(seeded_running_stats(seeded_state_dict(model.state_dict(), 0)))
    model.eval()
    runs = {}
    with torch.no_grad():
        for s in sorted(set(A.SUBSETS)):
            with G.Injector([eps], []):
                runs[s] = model([inputs[0] if s[0] else None, inputs[1] if s[1] else None], pose=inputs[2] if s[2] else None,
                                condition=cond)
    rows = A.row_subsets()
    pick = lambda k: torch.stack([runs[s][k][b] for b, s in enumerate(rows)])
    out[f"{tag}/means"] = pick(3).numpy()
    out[f"{tag}/log_var"] = pick(4).numpy()
    out[f"{tag}/pose"] = pick(2).numpy()
    out[f"{tag}/visual"] = np.stack([G.summarize(runs[s][0][b], 256) for b, s in enumerate(rows)])
    out[f"{tag}/tactile"] = np.stack([G.summarize(runs[s][1][b], 256) for b, s in enumerate(rows)])
    print(tag, out[f"{tag}/means"][:, 0])


if __name__ == "__main__":
    out = {"row_subset": np.array(A.row_subsets(), dtype=np.int64), "torch_version": torch.__version__}
    gen("plain", False, out)
    gen("cat", True, out)
    np.savez_compressed(os.path.join(HERE, "mixed_modal.npz"), **out)
    print("mixed_modal.npz", os.path.getsize(os.path.join(HERE, "mixed_modal.npz")), "bytes")
