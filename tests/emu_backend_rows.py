"""CPU emulation of the per-sample ELBO ops (mmdyn_*_rows*): :class:`tests.emu_backend.EmuBackend` plus the row ops of
``HipBackend``, restated with torch CPU ops.  Tests install it with ``ops.set_backend``; never imported by the product."""
import torch
import torch.nn.functional as F

from emu_backend import EmuBackend


class EmuBackendRows(EmuBackend):

    def bce_logits_rows_groups(self, logits, target, rows_out, slot_of_group, Bg, chw, mask=None, hw=0, mask_channels=1,
                               unmasked_rows=None):
        G = len(slot_of_group)
        lg, t = logits.reshape(G, Bg, chw), target.reshape(Bg, chw)
        mk = None
        if mask is not None:
            c = chw // hw
            assert mask_channels in (1, c) and mask.numel() == Bg * mask_channels * hw
            mk = mask.reshape(Bg, mask_channels, hw).expand(Bg, c, hw).reshape(Bg, chw)
        for g, slot in enumerate(slot_of_group):
            if slot < 0:
                continue
            x = lg[g]
            if mk is not None:
                rows_out[slot] += F.binary_cross_entropy_with_logits(x * mk, t * mk, reduction="none").double().sum(1)
                if unmasked_rows is not None:
                    unmasked_rows[slot] += F.binary_cross_entropy_with_logits(x, t, reduction="none").double().sum(1)
            else:
                rows_out[slot] += F.binary_cross_entropy_with_logits(x, t, reduction="none").double().sum(1)

    def tconv_out3_bn_bce_rows(self, y, mean, rstd, gamma, beta, w, logits, logits_group, target, loss_rows, slot_of_group, G, Bg,
                               Hi, Wi, mask=None, mask_channels=1, unmasked_rows=None):
        full = torch.empty(G * Bg, 3, 2 * Hi, 2 * Wi)
        EmuBackend.tconv_out3_bn_fwd(self, y, mean, rstd, gamma, beta, w, full, G, Bg, Hi, Wi)
        self.bce_logits_rows_groups(full, target, loss_rows, slot_of_group, Bg, target[0].numel(), mask=mask,
                                    hw=target[0, 0].numel(), mask_channels=mask_channels, unmasked_rows=unmasked_rows)
        if logits is not None:
            src = full if logits_group < 0 else full[logits_group * Bg:(logits_group + 1) * Bg]
            logits.reshape(-1).copy_(src.reshape(-1))

    def mse_rows_groups(self, r, t, rows_out, slot_of_group, Bg, n):
        G = len(slot_of_group)
        d = r.reshape(G, Bg, n) - t.reshape(1, Bg, n)
        for g, slot in enumerate(slot_of_group):
            rows_out[slot] += (d[g] * d[g]).double().sum(1)

    def kl_rows(self, mu, logvar, kl_rows, P, B, L):
        m, v = mu.reshape(P, B, L), logvar.reshape(P, B, L)
        kl_rows.reshape(P, B).copy_(-0.5 * (1 + v - m * m - v.exp()).double().sum(2))

    def elbo_assemble_rows(self, bce_rows, mse_rows, kl_rows, kl_sum, out, partials, P, B, kl_weight, pose_multiplier,
                           kl_weight_dev=None, kl_mode=0):
        if kl_weight_dev is not None:
            kl_weight = kl_weight * float(kl_weight_dev[0])
        v = torch.zeros(P, B, dtype=torch.float64)
        if bce_rows is not None:
            v += bce_rows.reshape(-1)[:P * B].reshape(P, B)
        if mse_rows is not None:
            v += pose_multiplier * mse_rows.reshape(-1)[:P * B].reshape(P, B)
        if kl_mode and kl_rows is not None:
            v += kl_weight * kl_rows.reshape(-1)[:P * B].reshape(P, B)
        if not kl_mode and kl_sum is not None:
            v += kl_weight * kl_sum.reshape(-1)[:P].reshape(P, 1)
        if partials is not None:
            partials.reshape(-1)[:P * B].copy_(v.reshape(-1).float())
        out.reshape(-1)[:B].copy_(v.sum(0).float())
