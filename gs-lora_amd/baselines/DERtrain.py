"""DERtrain — the epoch loop of the DER and DER++ baselines, MI355X-native counterpart of the reference's
`baselines/DERtrain.train_one_epoch_DER`: same name, same parameters in the same order with the same defaults, same 5-tuple, importable as
the reference's driver imports it:

    from baselines.DERtrain import train_one_epoch_DER

One step is gslora_hip.step.distill_step(method="der"): loss = CE_forget + lambda_der * ||emb_s(x_r) - emb_t(x_r)||_F^2, and with plus=True
(DER++) + lambda_der_plus * CE of a second remain batch drawn inside the step. The loop structure (with DER's extra None check in front of
the loop) and the deliberate differences are those of baselines/_distill.py. The reference keeps no meter for the DER++ cross-entropy;
neither does this loop.
"""
import torch

from baselines._distill import DISP_FREQ, VER_FREQ, DistillQueue, run_epoch  # noqa: F401


class DerQueue(DistillQueue):
    ORDER = ("losses_CE", "losses_DER", "_ce_next_unused", "losses_total")


def DER_regularzaion_loss(preds, gts):
    """torch.norm(preds - gts, p=2) squared, as the reference forms it (n = sqrt(sum), n * n), on the HIP kernels: gslora_hip.fd.row_dist in
    mode "sq" over all rows of `preds` ([B, D] f32 on the GPU). `gts` receives no gradient."""
    from gslora_hip.fd import row_dist
    return row_dist(preds, 0, preds.shape[0], gts, "sq", 1.0)[1]


def train_one_epoch_DER(student_model: torch.nn.Module, teacher_model: torch.nn.Module, data_loader_cl_forget, remain_loader,
                        criterion: torch.nn.Module, optimizer: torch.optim.Optimizer, device: torch.device, epoch: int, batch: int, losses_CE,
                        losses_DER, losses_total, task_i: str, testloader_forget, testloader_remain, forget_acc_before: float,
                        highest_H_mean: float, cfg: dict, lambda_der: float, plus: bool = False, lambda_der_plus: float = 0.0,
                        testloader_open=None):
    """One epoch over the forget loader. Returns (batch, highest_H_mean, losses_CE, losses_DER, losses_total)."""
    meters = dict(losses_CE=losses_CE, losses_DER=losses_DER, losses_total=losses_total)
    display = (("CE", "losses_CE"), ("DER", "losses_DER"), ("Total", "losses_total"))
    batch, highest_H_mean = run_epoch(student_model, teacher_model, data_loader_cl_forget, remain_loader, criterion, optimizer, device, epoch, batch,
                                      meters, DerQueue(), display, task_i, testloader_forget, testloader_remain, forget_acc_before, highest_H_mean,
                                      cfg, testloader_open, method="der", lam=lambda_der, lam_aux=lambda_der_plus, plus=bool(plus),
                                      check_first_draw=True)
    return batch, highest_H_mean, losses_CE, losses_DER, losses_total
