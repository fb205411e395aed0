"""CPU emulation of the ensemble rollout's quantile op (mmdyn_ensemble_quantiles): :class:`EmuBackendEnsemble` plus the one
operation, written here from the header's contract -- a rank per sample by counting (a smaller value, or an equal one with a smaller
index, is in front), a gather of the samples of rank lo and hi, one fp64 torch operation per step of the interpolation -- not the
sort of tests/quantile_cases.py.  Argument errors are ``ValueError``.  Tests install it with ``ops.set_backend``; never imported by
the product."""
import torch

from emu_backend_ensemble import EmuBackendEnsemble

QUANTILES_MAX, QUANTILE_N_MAX = 8, 128


class EmuBackendQuantiles(EmuBackendEnsemble):

    def ensemble_quantiles(self, groups, lo, frac, N, B):
        name = "mmdyn_hip: ensemble_quantiles: "
        if not isinstance(groups, (list, tuple)) or not 1 <= len(groups) <= 4:
            raise ValueError(name + "between 1 and 4 groups")
        if B < 1 or not 1 <= N <= QUANTILE_N_MAX:
            raise ValueError(name + f"B must be positive and N lie in [1, {QUANTILE_N_MAX}]")
        if len(lo) != len(frac) or not 1 <= len(lo) <= QUANTILES_MAX:
            raise ValueError(name + f"lo and frac of one length in [1, {QUANTILES_MAX}]")
        if any(isinstance(l, bool) or not isinstance(l, int) or not 0 <= l < N for l in lo) or \
                any(not 0.0 <= float(f) < 1.0 for f in frac):
            raise ValueError(name + "lo in [0, N) and frac in [0, 1)")
        Q = len(lo)
        for g in groups:
            src, out = g["src"], g["out"]
            row = tuple(src.shape[1:])
            if src.dtype != torch.float32 or out.dtype != torch.float32 or src.shape[0] != N * B or tuple(out.shape) != (Q, B) + row \
                    or src.numel() == 0:
                raise ValueError(name + "src [N * B, ...] and out [Q, B, ...] fp32 of one non-empty row shape")
        for g in groups:
            src, out = g["src"], g["out"]
            p = (torch.sigmoid(src) if g["logits"] else src).reshape(N, -1)
            idx = torch.arange(N).reshape(N, 1)
            rank = torch.zeros(p.shape, dtype=torch.int64)
            for m in range(N):
                rank += (p[m] < p) | ((p[m] == p) & (m < idx))
            nan = torch.isnan(p).any(0)
            for j in range(Q):
                hi = min(lo[j] + 1, N - 1)
                # the ranks of an element without NaN are a permutation: exactly one sample has rank lo (hi)
                take = lambda k: p.gather(0, (rank == k).to(torch.int64).argmax(0, keepdim=True))[0]
                a = take(lo[j])
                if frac[j] == 0.0:
                    r = a.clone()
                else:
                    a64, b64 = a.double(), take(hi).double()
                    r = torch.add(a64, torch.mul(torch.sub(b64, a64), float(frac[j]))).to(torch.float32)
                r = torch.where(nan, torch.full_like(r, float("nan")), r)
                out[j].copy_(r.reshape(out[j].shape))
