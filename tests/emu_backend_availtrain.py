"""CPU emulation of the ops of the training step on a mixed-modality batch (mmdyn_poe_bwd_avail_weighted, mmdyn_term_weights,
mmdyn_elbo_assemble_avail_weighted): :class:`EmuBackendRefine` (the most-derived emulation backend) plus the three operations
restated with torch from the header's contract -- ``torch.where``, never a product with the table, so what an absent entry holds (NaN,
Inf) cannot reach an output here either.  Tests install it with ``ops.set_backend``; never imported by the product."""
import torch

from emu_backend_avail import _table
from emu_backend_refine import EmuBackendRefine
from emu_backend_weighted import _w
from mmdyn_hip._lib import MmdynError


class EmuBackendAvailTrain(EmuBackendRefine):

    def poe_bwd_avail_weighted(self, passes, avail, eps_noise, mu, logvar, dz, g_mu, g_lv, kl_scale, w_kl, with_prior, P, B, L,
                               kl_weight_dev=None):
        """poe_bwd_avail's restatement with the KL term of row b scaled by kl_scale * w_kl[b]."""
        tabs = self._tables(avail, with_prior, P, B, "poe_bwd_avail_weighted")
        if kl_weight_dev is not None:
            kl_scale = kl_scale * float(kl_weight_dev[0])
        scale = kl_scale * _w(w_kl, B, "poe_bwd_avail_weighted")[:, None]
        for i, p in enumerate(passes):
            idx = [m for m in range(len(p["ld"])) if p["mu"][m] is not None]
            on = tabs[i]
            # (an absent word may hold anything: it is replaced before it enters the graph, as in EmuBackendAvail.poe_bwd_avail)
            sel = lambda t, m: t if on is None else torch.where(on[:, m:m + 1], t, torch.zeros_like(t))
            with torch.enable_grad():
                mus = [sel(p["mu"][m][:, :L].detach(), m).clone().requires_grad_(True) for m in idx]
                lvs = [sel(p["lv"][m][:, :L].detach(), m).clone().requires_grad_(True) for m in idx]
                pm, plv = self._poe_avail_math(p, on, with_prior, B, L, leaves=(mus, lvs))
                obj = (scale * (-0.5 * (1 + plv - pm * pm - plv.exp()))).sum()
                gz, has = torch.zeros(B, L), False
                if dz is not None:
                    gz, has = gz + dz.reshape(P, B, L)[i], True
                for t in p.get("dz", []):
                    if t is not None:
                        gz, has = gz + t.reshape(B, L), True
                if has:
                    obj = obj + ((eps_noise.reshape(P, B, L)[i] * torch.exp(0.5 * plv) + pm) * gz).sum()
                if g_mu is not None:
                    obj = obj + (pm * g_mu.reshape(P, B, L)[i]).sum()
                if g_lv is not None:
                    obj = obj + (plv * g_lv.reshape(P, B, L)[i]).sum()
                grads = torch.autograd.grad(obj, mus + lvs)
            for k, m in enumerate(idx):
                p["dmu"][m][:, :L] = sel(grads[k], m)
                p["dlv"][m][:, :L] = sel(grads[len(idx) + k], m)

    def term_weights(self, tavail, w, w_term, B):
        if w_term is None or w_term.dtype != torch.float32 or tuple(w_term.shape) != (3, B) or not w_term.is_contiguous():
            raise ValueError(f"mmdyn_term_weights: w_term must be a contiguous fp32 [3][B={B}] tensor")
        on = _table(tavail, B, "term_weights")
        wb = torch.ones(B) if w is None else _w(w, B, "term_weights")
        for m in range(3):
            w_term[m] = wb if on is None else torch.where(on[:, m], wb, torch.zeros(B))

    def elbo_assemble_avail_weighted(self, bce_v_rows, bce_t_rows, mse_rows, kl_rows, kl_sum, w, tavail, loss, wpartials, out, partials,
                                     w_sum_out, present, term_sums, P, B, kl_weight, pose_multiplier, kl_weight_dev=None, kl_mode=0):
        name = "elbo_assemble_avail_weighted"
        if P < 1 or P > 8 or B < 1 or (bce_v_rows is not None and bce_v_rows is bce_t_rows):
            raise MmdynError(f"mmdyn_{name} failed: MMDYN_ERR_SHAPE (unsupported dimensions)")
        on = _table(tavail, B, name)
        if kl_weight_dev is not None:
            kl_weight = kl_weight * float(kl_weight_dev[0])
        wd = torch.ones(B, dtype=torch.float64) if w is None else _w(w, B, name).double()
        zero = torch.zeros(P, B, dtype=torch.float64)
        terms = []
        for m, rows in enumerate((bce_v_rows, bce_t_rows, mse_rows)):
            if rows is None:
                terms.append(zero)
                continue
            tab = rows.reshape(-1)[:P * B].reshape(P, B)
            if on is not None:           # the table entry of an absent target is overwritten with 0, whatever it held
                tab.copy_(torch.where(on[:, m][None, :], tab, zero))
            terms.append(tab)
        rec = (terms[0] + terms[1]) + pose_multiplier * terms[2]
        klr = zero if kl_rows is None else kl_rows.reshape(-1)[:P * B].reshape(P, B)
        kls = torch.zeros(P, dtype=torch.float64) if kl_sum is None else kl_sum.reshape(-1)[:P]
        kl = klr if kl_mode else kls[:, None].expand(P, B)
        v = rec + kl_weight * kl
        if partials is not None:
            partials.reshape(-1)[:P * B].copy_(v.reshape(-1).float())
        if out is not None:
            out.reshape(-1)[:B].copy_(v.sum(0).float())
        wp = ((rec * wd).sum(1) + kl_weight * ((klr * wd).sum(1) if kl_mode else wd.sum() * kls)) / B
        if wpartials is not None:
            wpartials.reshape(-1)[:P].copy_(wp.float())
        loss[0] = float(wp.sum())
        if w_sum_out is not None:
            w_sum_out.fill_(float(wd.sum()))
        if present is not None:
            present.reshape(-1)[:3].copy_(torch.full((3,), float(B), dtype=torch.float64) if on is None else on[:, :3].double().sum(0))
        if term_sums is not None:
            term_sums.reshape(-1)[:3 * P].copy_(torch.stack([t.sum(1) for t in terms]).reshape(-1))
