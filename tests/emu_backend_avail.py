"""CPU emulation of the per-row availability ops (mmdyn_poe_fwd_avail / _bwd_avail, mmdyn_complete_select,
mmdyn_elbo_assemble_rows_avail): :class:`EmuBackendCond` plus the three operations restated with torch -- ``torch.where``, never a
multiplication by the mask, so an absent word that holds NaN / Inf cannot reach an output here either.  Tests install it with
``ops.set_backend``; never imported by the product."""
import torch

from emu_backend_cond import EmuBackendCond
from mmdyn_hip._lib import MmdynError


def _table(t, B, name):
    if t is None:
        return None
    if t.dtype != torch.uint8 or tuple(t.shape) != (B, 4) or not t.is_contiguous():
        raise ValueError(f"mmdyn_hip: {name}: the availability table must be a contiguous uint8 [B={B}][4] tensor")
    return t != 0


class EmuBackendAvail(EmuBackendCond):

    def _poe_avail_math(self, p, on, with_prior, B, L, leaves=None):
        """The arithmetic of EmuBackend._poe_math, an expert's terms selected per row.  on: bool [B][4] or None."""
        eps = 1e-8
        sumT = torch.ones(B, L) / ((torch.ones(B, L) + eps) + eps) if with_prior else torch.zeros(B, L)
        sumMuT = torch.zeros(B, L)
        k = 0
        for m in range(len(p["ld"])):
            if p["mu"][m] is None:
                continue
            mu, lv = (leaves[0][k], leaves[1][k]) if leaves is not None else (p["mu"][m][:, :L], p["lv"][m][:, :L])
            k += 1
            T = 1.0 / ((torch.exp(lv) + eps) + eps)
            if on is None:
                sumT, sumMuT = sumT + T, sumMuT + mu * T
            else:
                row = on[:, m:m + 1]
                sumT = torch.where(row, sumT + T, sumT)
                sumMuT = torch.where(row, sumMuT + mu * T, sumMuT)
        return sumMuT / sumT, torch.log(1.0 / sumT + eps)

    @staticmethod
    def _tables(avail, with_prior, P, B, name):
        tabs = [None] * P if avail is None else [_table(t, B, name) for t in avail]
        if len(tabs) != P:
            raise ValueError(f"mmdyn_hip: {name}: {len(tabs)} availability tables for {P} passes")
        if not with_prior and any(t is not None for t in tabs):
            raise MmdynError(f"mmdyn_{name} failed: MMDYN_ERR_SHAPE (unsupported dimensions)")
        return tabs

    def poe_fwd_avail(self, passes, avail, eps_noise, mu, logvar, z, kl_sum, with_prior, P, B, L):
        tabs = self._tables(avail, with_prior, P, B, "poe_fwd_avail")
        for i, p in enumerate(passes):
            pm, plv = self._poe_avail_math(p, tabs[i], with_prior, B, L)
            mu.reshape(P, B, L)[i] = pm
            logvar.reshape(P, B, L)[i] = plv
            if z is not None:
                z.reshape(P, B, L)[i] = eps_noise.reshape(P, B, L)[i] * torch.exp(0.5 * plv) + pm
                for t in p.get("zdst", []):
                    if t is not None:
                        t.reshape(B, L).copy_(z.reshape(P, B, L)[i])
            if kl_sum is not None:
                kl_sum[i] += (-0.5 * (1 + plv - pm * pm - plv.exp()).double().sum())

    def poe_bwd_avail(self, passes, avail, eps_noise, mu, logvar, dz, g_mu, g_lv, kl_scale, with_prior, P, B, L, kl_weight_dev=None):
        tabs = self._tables(avail, with_prior, P, B, "poe_bwd_avail")
        if kl_weight_dev is not None:
            kl_scale = kl_scale * float(kl_weight_dev[0])
        for i, p in enumerate(passes):
            idx = [m for m in range(len(p["ld"])) if p["mu"][m] is not None]
            on = tabs[i]
            # an absent word may hold anything: it is replaced before it enters the graph (where() alone would still send NaN * 0
            # through the backward of the unselected branch)
            sel = lambda t, m: t if on is None else torch.where(on[:, m:m + 1], t, torch.zeros_like(t))
            with torch.enable_grad():
                mus = [sel(p["mu"][m][:, :L].detach(), m).clone().requires_grad_(True) for m in idx]
                lvs = [sel(p["lv"][m][:, :L].detach(), m).clone().requires_grad_(True) for m in idx]
                pm, plv = self._poe_avail_math(p, on, with_prior, B, L, leaves=(mus, lvs))
                obj = kl_scale * (-0.5 * (1 + plv - pm * pm - plv.exp()).sum())
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

    def complete_select(self, x, recon, avail, modality, out, logits):
        B = recon.shape[0]
        fill = torch.sigmoid(recon) if logits else recon
        if x is None:
            out.copy_(fill)
            return
        on = _table(avail, B, "complete_select")
        row = torch.ones(B, dtype=torch.bool) if on is None else on[:, modality]
        out.copy_(torch.where(row.reshape((B,) + (1,) * (recon.dim() - 1)), x, fill))

    def elbo_assemble_rows_avail(self, bce_rows, mse_rows, kl_rows, kl_sum, out, partials, avail, bce_modality, mse_modality, P, B,
                                 kl_weight, pose_multiplier, kl_weight_dev=None, kl_mode=0):
        on = _table(avail, B, "elbo_assemble_rows_avail")
        for rows, modal in ((bce_rows, bce_modality), (mse_rows, mse_modality)):
            if rows is None:
                continue
            tab = rows.reshape(-1)[:P * B].reshape(P, B)
            for p in range(P):
                if modal[p] >= 0:
                    tab[p] = torch.where(on[:, modal[p]], tab[p], torch.zeros_like(tab[p]))
        self.elbo_assemble_rows(bce_rows, mse_rows, kl_rows, kl_sum, out, partials, P, B, kl_weight, pose_multiplier,
                                kl_weight_dev=kl_weight_dev, kl_mode=kl_mode)
