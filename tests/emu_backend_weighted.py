"""CPU emulation of the weighted-ELBO ops (mmdyn_*_rows_groups_grad, mmdyn_tconv_out3_bn_bce_rows_grad, mmdyn_poe_bwd_weighted,
mmdyn_reparam_bwd_weighted, mmdyn_elbo_assemble_weighted): :class:`EmuBackendAvail` plus those operations restated with torch.
Tests install it with ``ops.set_backend``; never imported by the product."""
import torch

from emu_backend import EmuBackend
from emu_backend_avail import EmuBackendAvail


def _w(w, B, name):
    if w is None or w.dtype != torch.float32 or w.numel() != B or not w.is_contiguous():
        raise ValueError(f"mmdyn_hip: {name}: the weights must be a contiguous fp32 vector of B={B} elements")
    return w.reshape(B)


class EmuBackendWeighted(EmuBackendAvail):

    def bce_logits_rows_groups_grad(self, logits, target, dlogit, w_rec, rows_out, slot_of_group, Bg, chw, grad_scale, mask=None,
                                    hw=0, mask_channels=1, unmasked_rows=None):
        G = len(slot_of_group)
        w = _w(w_rec, Bg, "bce_logits_rows_groups_grad")
        self.bce_logits_rows_groups(logits, target, rows_out, slot_of_group, Bg, chw, mask=mask, hw=hw, mask_channels=mask_channels,
                                    unmasked_rows=unmasked_rows)
        lg, t, dl = logits.reshape(G, Bg, chw), target.reshape(Bg, chw), dlogit.reshape(G, Bg, chw)
        mk = None
        if mask is not None:
            c = chw // hw
            mk = mask.reshape(Bg, mask_channels, hw).expand(Bg, c, hw).reshape(Bg, chw)
        for g, slot in enumerate(slot_of_group):
            if slot < 0:
                dl[g].zero_()
            elif mk is None:
                dl[g] = ((torch.sigmoid(lg[g]) - t) * grad_scale) * w[:, None]
            else:
                dl[g] = (mk * (torch.sigmoid(lg[g] * mk) - t * mk) * grad_scale) * w[:, None]

    def tconv_out3_bn_bce_rows_grad(self, y, mean, rstd, gamma, beta, w, logits, logits_group, target, dlogit, w_rec, loss_rows,
                                    slot_of_group, grad_scale, G, Bg, Hi, Wi, mask=None, mask_channels=1, unmasked_rows=None):
        full = torch.empty(G * Bg, 3, 2 * Hi, 2 * Wi)
        EmuBackend.tconv_out3_bn_fwd(self, y, mean, rstd, gamma, beta, w, full, G, Bg, Hi, Wi)
        self.bce_logits_rows_groups_grad(full, target, dlogit, w_rec, loss_rows, slot_of_group, Bg, target[0].numel(), grad_scale,
                                         mask=mask, hw=target[0, 0].numel(), mask_channels=mask_channels,
                                         unmasked_rows=unmasked_rows)
        if logits is not None:
            src = full if logits_group < 0 else full[logits_group * Bg:(logits_group + 1) * Bg]
            logits.reshape(-1).copy_(src.reshape(-1))

    def mse_rows_groups_grad(self, r, t, dr, w_rec, rows_out, slot_of_group, Bg, n, grad_scale):
        G = len(slot_of_group)
        w = _w(w_rec, Bg, "mse_rows_groups_grad")
        self.mse_rows_groups(r, t, rows_out, slot_of_group, Bg, n)
        d = r.reshape(G, Bg, n) - t.reshape(1, Bg, n)
        dr.reshape(G, Bg, n).copy_((2 * d * grad_scale) * w[None, :, None])

    def poe_bwd_weighted(self, passes, eps_noise, mu, logvar, dz, g_mu, g_lv, kl_scale, w_kl, with_prior, P, B, L,
                         kl_weight_dev=None):
        if kl_weight_dev is not None:
            kl_scale = kl_scale * float(kl_weight_dev[0])
        # (EmuBackend._poe_bwd multiplies the KL sum by kl_scale: a [B][1] tensor weights it per row)
        scale = kl_scale * _w(w_kl, B, "poe_bwd_weighted")[:, None]
        with torch.enable_grad():
            self._poe_bwd_rows(passes, eps_noise, mu, logvar, dz, g_mu, g_lv, scale, with_prior, P, B, L)

    def _poe_bwd_rows(self, passes, eps_noise, mu, logvar, dz, g_mu, g_lv, scale, with_prior, P, B, L):
        for i, p in enumerate(passes):
            idx = [m for m in range(len(p["ld"])) if p["mu"][m] is not None]
            mus = [p["mu"][m][:, :L].detach().clone().requires_grad_(True) for m in idx]
            lvs = [p["lv"][m][:, :L].detach().clone().requires_grad_(True) for m in idx]
            pm, plv = self._poe_math(mus, lvs, with_prior, B, L)
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
                p["dmu"][m][:, :L] = grads[k]
                p["dlv"][m][:, :L] = grads[len(idx) + k]

    def reparam_bwd_weighted(self, mu, lv, eps_noise, dz, kl_scale, w_kl, dmu, dlv, B, L, ld):
        s = kl_scale * _w(w_kl, B, "reparam_bwd_weighted")[:, None]
        m, v = mu[:, :L], lv[:, :L]
        gm = s * m
        gv = -0.5 * s * (1 - v.exp())
        if dz is not None:
            gm = gm + dz.reshape(B, L)
            gv = gv + dz.reshape(B, L) * eps_noise.reshape(B, L) * 0.5 * torch.exp(0.5 * v)
        dmu[:, :L] = gm
        dlv[:, :L] = gv

    def elbo_assemble_weighted(self, bce_rows, mse_rows, kl_rows, kl_sum, w, loss, wpartials, out, partials, w_sum_out, P, B,
                               kl_weight, pose_multiplier, kl_weight_dev=None, kl_mode=0):
        if kl_weight_dev is not None:
            kl_weight = kl_weight * float(kl_weight_dev[0])
        wd = _w(w, B, "elbo_assemble_weighted").double()
        tab = lambda t: torch.zeros(P, B, dtype=torch.float64) if t is None else t.reshape(-1)[:P * B].reshape(P, B)
        rec = tab(bce_rows) + pose_multiplier * tab(mse_rows)
        klr = tab(kl_rows)
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
