"""FDRtrain — the epoch loop of the FDR baseline (function-distance regularisation), MI355X-native counterpart of the reference's
`baselines/FDRtrain.train_one_epoch_FDR`: same name, same parameters in the same order (criterion is the THIRD one here, as in the
reference) with the same default, same 5-tuple, importable as the reference's driver imports it:

    from baselines.FDRtrain import train_one_epoch_FDR

One step is gslora_hip.step.distill_step(method="fdr"): loss = CE_forget + reg_lambda * mean_b ||logits_s(x_r)_b - logits_t(x_r)_b||_2. The
loop structure and the deliberate differences are those of baselines/_distill.py.
"""
import torch

from baselines._distill import DISP_FREQ, VER_FREQ, DistillQueue, run_epoch  # noqa: F401


class FdrQueue(DistillQueue):
    ORDER = ("losses_CE", "losses_FDR", "_aux_unused", "losses_total")


def regularization_loss(outputs, target_logits):
    """torch.norm(outputs - target_logits, 2, 1).mean() on the HIP kernels: gslora_hip.fd.row_dist in mode "rownorm" over all rows of
    `outputs` ([B, C] f32 on the GPU). A row that equals its target has an exactly zero gradient (torch.norm's subgradient at 0);
    `target_logits` receives no gradient."""
    from gslora_hip.fd import row_dist
    return row_dist(outputs, 0, outputs.shape[0], target_logits, "rownorm", 1.0)[1]


def train_one_epoch_FDR(student_model: torch.nn.Module, teacher_model: torch.nn.Module, criterion: torch.nn.Module, data_loader_cl_forget,
                        remain_loader, optimizer: torch.optim.Optimizer, device: torch.device, epoch: int, batch: int, losses_CE, losses_FDR,
                        losses_total, reg_lambda: float, task_i: str, testloader_forget, testloader_remain, forget_acc_before: float,
                        highest_H_mean: float, cfg: dict, testloader_open=None):
    """One epoch over the forget loader. Returns (batch, highest_H_mean, losses_CE, losses_FDR, losses_total)."""
    criterion.train()
    meters = dict(losses_CE=losses_CE, losses_FDR=losses_FDR, losses_total=losses_total)
    display = (("CE", "losses_CE"), ("FDR", "losses_FDR"), ("Total", "losses_total"))
    batch, highest_H_mean = run_epoch(student_model, teacher_model, data_loader_cl_forget, remain_loader, criterion, optimizer, device, epoch, batch,
                                      meters, FdrQueue(), display, task_i, testloader_forget, testloader_remain, forget_acc_before, highest_H_mean,
                                      cfg, testloader_open, method="fdr", lam=reg_lambda)
    return batch, highest_H_mean, losses_CE, losses_FDR, losses_total
