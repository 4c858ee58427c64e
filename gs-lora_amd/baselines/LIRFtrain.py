"""LIRFtrain — the epoch loop of the LIRF baseline, MI355X-native counterpart of the reference's `baselines/LIRFtrain.py`: the same
names, the same parameters in the same order with the same defaults, the same return arity, importable as the reference's driver imports
them:

    from baselines.LIRFtrain import train_one_epoch_LIRF, eval_data_LIRF

One step is gslora_hip.step.lirf_step (the student's lower half and the shared upper half as one pass, the attention-transfer term on the
mid stream through libgslora_at.so). The structure is the reference's: a remain prefetcher that restarts when exhausted, one step per
forget batch, display every DISP_FREQ = 5 steps with the six meters reset in place, evaluate_LIRF every VER_FREQ = 5 steps, the next
remain batch drawn at the end of the step. Differences that are deliberate, as in the other baseline loops:
  * one deferred host sync per display interval instead of six `.item()` per step (meter values are identical);
  * wandb is optional, as in engine_cl;
  * the trainable set and the deposit network: see lirf_step's docstring.
at, at_loss and AT are the reference's names on the HIP kernels: forward values only, NOT differentiable.
"""
import torch
import torch.nn as nn

from engine_cl import EVAL_DTYPE, _EVAL_SAME, _log
from gslora_hip.step import MeterQueue, lirf_step
from util.data_prefetcher import data_prefetcher

DISP_FREQ = 5
VER_FREQ = 5


class LirfQueue(MeterQueue):
    """MeterQueue over lirf_step's [CE, AT, KP, PT_RE, total, REPLAY] packs; every meter is weighted with the forget batch's size, as in the
    reference (:155-160)."""
    ORDER = ("losses_CE", "losses_AT", "kd_lossesKP", "losses_pt_re", "losses_total", "losses_remain")
    WEIGHT = ("f",) * 6


def at(x):
    """The reference's at(x) on a [B, T, D] stream -> [B, D] f32 (gslora_hip.at.at: the forward value only, not differentiable)."""
    from gslora_hip.at import at as _at
    return _at(x)


def at_loss(x, y):
    """The reference's at_loss(x, y) on two [B, T, D] streams -> a 0-dim f32 device tensor (gslora_hip.at.at_loss: the forward value only,
    not differentiable; a training step takes the gradient through gslora_hip.step.lirf_step)."""
    from gslora_hip.at import at_loss as _at_loss
    return _at_loss(x, y)


class AT(nn.Module):
    """The reference's AT module (:17-39, p = 2) is built by its loop and never called (the loss line uses at_loss). Same constructor; a
    call is refused: its 4-D feature-map form has no kernel here."""

    def __init__(self):
        super().__init__()
        self.p = 2

    def forward(self, fm_s, fm_t):
        raise NotImplementedError("gs-lora_amd: AT.forward (the 4-D feature-map form) is never called by the LIRF loop; the loss of the "
                                  "[B, T, D] stream is baselines.LIRFtrain.at_loss")


def train_one_epoch_LIRF(student_low: torch.nn.Module, deposit_low: torch.nn.Module, teacher_low: torch.nn.Module,
                         teacher_up: torch.nn.Module, data_loader_cl_forget, remain_loader, criterion: torch.nn.Module,
                         optimizer: torch.optim.Optimizer, device: torch.device, epoch: int, batch: int, losses_CE, losses_AT, kd_lossesKP,
                         losses_pt_re, losses_total, losses_remain, task_i: str, testloader_forget, testloader_remain,
                         forget_acc_before: float, highest_H_mean: float, cfg: dict, testloader_open=None):
    """One epoch over the forget loader. Returns (batch, highest_H_mean, losses_CE, losses_AT, kd_lossesKP, losses_pt_re, losses_total,
    losses_remain)."""
    student_low.train()
    deposit_low.train()
    criterion.train()
    teacher_low.eval()
    teacher_up.eval()
    meters = dict(losses_CE=losses_CE, losses_AT=losses_AT, kd_lossesKP=kd_lossesKP, losses_pt_re=losses_pt_re, losses_total=losses_total,
                  losses_remain=losses_remain)
    queue = LirfQueue()
    split, T, alpha = cfg["PER_FORGET_CLS"], cfg["LIRF_T"], cfg["LIRF_alpha"]
    prefetcher_remain = data_prefetcher(remain_loader, device=device, prefetch=True)
    inputs_remain, labels_remain = prefetcher_remain.next()
    for inputs_forget, labels_forget in iter(data_loader_cl_forget):
        inputs_forget, labels_forget = inputs_forget.to(device), labels_forget.to(device)
        pack = lirf_step(student_low, deposit_low, teacher_low, teacher_up, optimizer, criterion, inputs_forget, labels_forget, inputs_remain,
                         labels_remain, split=split, T=T, alpha=alpha)
        queue.push(pack, inputs_forget.size(0), inputs_forget.size(0))
        if ((batch + 1) % DISP_FREQ == 0) and batch != 0:
            queue.flush(meters)
            _log({"epoch_loss_CE-{}".format(task_i): losses_CE.avg, "epoch_loss_AT-{}".format(task_i): losses_AT.avg,
                  "epoch_loss_kdKP-{}".format(task_i): kd_lossesKP.avg, "epoch_loss_pt_re-{}".format(task_i): losses_pt_re.avg,
                  "epoch_loss_total-{}".format(task_i): losses_total.avg, "epoch_loss_remain-{}".format(task_i): losses_remain.avg})
            print("Task {} Epoch {} Batch {}\t"
                  "Training CE Loss {loss_CE.val:.4f} ({loss_CE.avg:.4f})\t"
                  "Training AT Loss {loss_AT.val:.4f} ({loss_AT.avg:.4f})\t"
                  "Training total Loss {loss_total.val:.4f} ({loss_total.avg:.4f})\t"
                  "Training remain Loss {loss_remain.val:.4f} ({loss_remain.avg:.4f})\t".format(
                      task_i, epoch + 1, batch + 1, loss_CE=losses_CE, loss_AT=losses_AT, loss_total=losses_total, loss_remain=losses_remain))
            for m in meters.values():
                m.reset()
        with torch.no_grad():
            if ((batch + 1) % VER_FREQ == 0) and batch != 0:
                highest_H_mean = evaluate_LIRF(student_low, teacher_up, testloader_forget, testloader_remain, device, batch, epoch, task_i,
                                               forget_acc_before, highest_H_mean, cfg, optimizer, testloader_open=testloader_open)
                student_low.train()
        batch += 1
        inputs_remain, labels_remain = prefetcher_remain.next()
        if inputs_remain is None:      # the remain loader is exhausted: start it again
            prefetcher_remain = data_prefetcher(remain_loader, device=device, prefetch=True)
            inputs_remain, labels_remain = prefetcher_remain.next()
    queue.flush(meters)
    return batch, highest_H_mean, losses_CE, losses_AT, kd_lossesKP, losses_pt_re, losses_total, losses_remain


def eval_data_LIRF(student_low: torch.nn.Module, teacher_up: torch.nn.Module, testloader, device: torch.device, mode: str, batch: int = 0):
    """Accuracy (0-100) of teacher_up(student_low(images), labels) in eval mode, the margin applied because labels are passed, as the
    reference does (:250-282). Hits are counted on the device, one host read at the end. Like engine_cl.eval_data the accuracies are taken
    in f32 whatever mode the halves train in (GSLORA_EVAL_DTYPE); both halves return to their mode afterwards."""
    from gslora_hip import ops
    student_low.eval()
    teacher_up.eval()
    nets = [m.module if isinstance(m, nn.DataParallel) else m for m in (student_low, teacher_up)]
    before = [getattr(n, "compute_mode", None) for n in nets]
    switch = EVAL_DTYPE not in _EVAL_SAME and all(hasattr(n, "set_compute_dtype") for n in nets)
    if switch:
        for n in nets:
            n.set_compute_dtype(EVAL_DTYPE)
    hits, total = None, 0
    try:
        with torch.no_grad():
            for images, labels in testloader:
                images, labels = images.to(device), labels.to(device).long()
                outputs, _ = teacher_up(student_low(images), labels)
                h = ops.ce_fwd(outputs.float().contiguous(), labels.contiguous())[1]
                hits = h if hits is None else hits + h
                total += labels.size(0)
    finally:
        if switch:
            for n, mode_name in zip(nets, before):
                n.set_compute_dtype(mode_name)
    accuracy = 100 * (hits.item() if hits is not None else 0.0) / max(total, 1)
    print("Test {} Accuracy in LIRF = {:.2f}%".format(mode, accuracy))
    _log({"Test {} Accuracy".format(mode): accuracy})
    return accuracy


def evaluate_LIRF(student_low: torch.nn.Module, teacher_up: torch.nn.Module, testloader_forget, testloader_remain, device: torch.device,
                  batch: int, epoch: int, task_i: str, forget_acc_before: float, highest_H_mean: float, cfg: dict,
                  optimizer: torch.optim.Optimizer, testloader_open=None):
    """Eval-mode accuracies and the H-mean 2 * drop * remain / (drop + remain + 1e-8), drop = forget_acc_before - forget_acc; returns the
    highest H-mean so far (reference :285-341: no checkpoint is written)."""
    student_low.eval()
    teacher_up.eval()
    lr = optimizer.param_groups[0]["lr"]
    print("current learning rate:{:.7f}".format(lr))
    print("Perfom evaluation on test set and save checkpoints...")
    forget_acc = eval_data_LIRF(student_low, teacher_up, testloader_forget, device, "forget-{}".format(task_i), batch)
    remain_acc = eval_data_LIRF(student_low, teacher_up, testloader_remain, device, "remain-{}".format(task_i), batch)
    if testloader_open is not None:
        eval_data_LIRF(student_low, teacher_up, testloader_open, device, "open-{}".format(task_i), batch)
    forget_drop = forget_acc_before - forget_acc
    Hmean = 2 * forget_drop * remain_acc / (forget_drop + remain_acc + 1e-8)
    if Hmean > highest_H_mean:
        highest_H_mean = Hmean
    return highest_H_mean
