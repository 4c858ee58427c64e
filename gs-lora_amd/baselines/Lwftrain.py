"""Lwftrain — the epoch loop of the LwF baseline, MI355X-native counterpart of the reference's `baselines/Lwftrain.train_one_epoch_Lwf`:
same name, same parameters in the same order with the same default, same 6-tuple, importable as the reference's driver imports it:

    from baselines.Lwftrain import train_one_epoch_Lwf

One step is gslora_hip.step.distill_step(method="lwf"): loss = CE_forget + lambda_kd * KD + lambda_remain * CE_remain, where KD is the
reference's L_old_kd_loss AS IT SHIPS — see L_old_kd_loss below: an exact 0 with an exact zero gradient, so the teacher is not run and the KD
meter reads 0. The loop structure and the deliberate differences are those of baselines/_distill.py.
"""
import torch

from baselines._distill import DISP_FREQ, VER_FREQ, DistillQueue, run_epoch  # noqa: F401


class LwfQueue(DistillQueue):
    ORDER = ("losses_CE", "losses_KD", "losses_remain", "losses_total")


def L_old_kd_loss(preds, gts, temperature=2.0):
    """The value the reference's function of this name returns: an exact 0. The reference forms l_preds = log_softmax(softmax(preds) **
    (1 / T)), which is <= 0 in every element, then takes torch.log of it — NaN where l_preds < 0, -inf where it is 0, and with at least two
    classes no element of a log_softmax is 0 — and sets every NaN to 0.0 before the sum with l_gts. For finite logits of two or more
    classes the value is therefore exactly 0.0 and the gradient to `preds` exactly zero (checked on CPU for 2, 10 and 1000 classes; DESIGN.md
    section 9n). The reference's behaviour is reproduced, not the paper's. One class is refused: the reference's value is NaN there.
    -> a 0-dim f32 zero on preds' device, without a gradient."""
    if preds.dim() < 1 or preds.shape != gts.shape:
        raise ValueError(f"L_old_kd_loss: predictions {tuple(preds.shape)} and targets {tuple(gts.shape)} differ in shape")
    if preds.shape[-1] < 2:
        raise ValueError(f"L_old_kd_loss: num_class >= 2 is required (the reference's value is NaN for one class), got {preds.shape[-1]}")
    return torch.zeros((), device=preds.device, dtype=torch.float32)


def train_one_epoch_Lwf(student_model: torch.nn.Module, teacher_model: torch.nn.Module, data_loader_cl_forget, remain_loader,
                        criterion: torch.nn.Module, optimizer: torch.optim.Optimizer, device: torch.device, epoch: int, batch: int, losses_CE,
                        losses_KD, losses_total, losses_remain, task_i: str, testloader_forget, testloader_remain, forget_acc_before: float,
                        highest_H_mean: float, cfg: dict, lambda_kd: float, lambda_remain: float, temperature: float, testloader_open=None):
    """One epoch over the forget loader. Returns (batch, highest_H_mean, losses_CE, losses_KD, losses_remain, losses_total). `temperature`
    and `lambda_kd` reach a term that is identically zero (L_old_kd_loss)."""
    meters = dict(losses_CE=losses_CE, losses_KD=losses_KD, losses_remain=losses_remain, losses_total=losses_total)
    display = (("CE", "losses_CE"), ("KD", "losses_KD"), ("Remain", "losses_remain"), ("Total", "losses_total"))
    batch, highest_H_mean = run_epoch(student_model, teacher_model, data_loader_cl_forget, remain_loader, criterion, optimizer, device, epoch, batch,
                                      meters, LwfQueue(), display, task_i, testloader_forget, testloader_remain, forget_acc_before, highest_H_mean,
                                      cfg, testloader_open, method="lwf", lam=lambda_kd, lam_aux=lambda_remain)
    return batch, highest_H_mean, losses_CE, losses_KD, losses_remain, losses_total
