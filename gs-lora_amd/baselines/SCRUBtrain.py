"""SCRUBtrain — the superepoch loop of the SCRUB baseline, MI355X-native counterpart of the reference's
`baselines/SCRUBtrain.train_one_superepoch_SCRUB`: same name, same 26 parameters with the same defaults, same 8-tuple, importable as the reference's driver imports
it:

    from baselines.SCRUBtrain import train_one_superepoch_SCRUB

The structure is the reference's: ten inner epochs; the first five run a pass over the forget loader with max steps (ascend the
distillation KL) and then a pass over the remain loader with min steps (CE + KL); the last five run min steps only, with `evaluate` every
VER_FREQ steps; `adjust_learning_rate(superepoch * 15 + i, cfg, optimizer)` at the head of each inner epoch; one
`swa_model.update_parameters(student)` at the end. The loop body is gslora_hip.step.scrub_step; the parameter distance is prepared once per
call as a gslora_hip.kd.ParamDist. Differences that are deliberate:
  * one deferred host sync per display interval instead of two or three `.item()` per step (meter values are identical);
  * wandb is optional, as in engine_cl;
  * the student is a ViT_face / ViTs_face built with lora_rank = 0 under the --only_ffn rule, one process, eager (scrub_step refuses the
    rest by name).
"""
import torch

from engine_cl import _log, evaluate
from gslora_hip.step import MeterQueue, scrub_step
from util.sgda_utils import adjust_learning_rate as sgda_adjust_learning_rate

DISP_FREQ = 5
VER_FREQ = 100


class ScrubForgetQueue(MeterQueue):
    """MeterQueue over the max steps' [kd, ce (not kept), total] packs, weighted with the batch size."""
    ORDER = ("losses_kd_forget", "_ce_unused", "losses_total_forget")
    WEIGHT = ("r", "r", "r")


class ScrubRemainQueue(MeterQueue):
    """MeterQueue over the min steps' [kd, ce, total] packs, weighted with the batch size."""
    ORDER = ("losses_kd_remain", "losses_CE", "losses_total_remain")
    WEIGHT = ("r", "r", "r")


def train_one_superepoch_SCRUB(student: torch.nn.Module, teacher: torch.nn.Module, swa_model: torch.nn.Module, data_loader_forget,
                               remain_loader, criterion: torch.nn.Module, optimizer: torch.optim.Optimizer, device: torch.device,
                               superepoch: int, batch: int, losses_CE, losses_total_forget, losses_total_remain, losses_kd_remain,
                               losses_kd_forget, task_i: str, testloader_forget, testloader_remain, forget_acc_before: float,
                               highest_H_mean: float, cfg: dict, kd_T: float = 2.0, sgda_smoothing: float = 0.0, sgda_gamma: float = 0.99,
                               sgda_alpha: float = 0.001, testloader_open=None):
    """One superepoch. Returns (batch, highest_H_mean, losses_CE, losses_total_forget, losses_total_remain, losses_kd_forget,
    losses_kd_remain, swa_model). The meters are reset in place after each display, as in the reference."""
    from gslora_hip.kd import ParamDist
    student.train()
    teacher.eval()
    criterion.train()
    dist = ParamDist(student, swa_model, sgda_smoothing)
    hyper = dict(kd_T=kd_T, sgda_gamma=sgda_gamma, sgda_alpha=sgda_alpha, dist=dist)
    meters = dict(losses_CE=losses_CE, losses_total_forget=losses_total_forget, losses_total_remain=losses_total_remain,
                  losses_kd_remain=losses_kd_remain, losses_kd_forget=losses_kd_forget)
    forget_q, remain_q = ScrubForgetQueue(), ScrubRemainQueue()

    def display(queue, side, names, epoch):
        queue.flush(meters)
        _log({"epoch_loss_{}-{}".format(n[len("losses_"):], task_i): meters[n].avg for n in names})
        print("Task {} Epoch {} Batch {}\t".format(task_i, epoch + 1, batch + 1)
              + "".join("{} Training {} Loss {:.4f} ({:.4f})\t".format(side, n.split("_")[1], meters[n].val, meters[n].avg) for n in names))
        for n in names:
            meters[n].reset()

    def one_pass(loader, maximize, epoch, verify):
        nonlocal batch, highest_H_mean
        queue, side = (forget_q, "Forget") if maximize else (remain_q, "Remain")
        names = ("losses_kd_forget", "losses_total_forget") if maximize else ("losses_kd_remain", "losses_total_remain", "losses_CE")
        for inputs, labels in iter(loader):
            inputs, labels = inputs.to(device), labels.to(device)
            queue.push(scrub_step(student, teacher, optimizer, criterion, inputs, labels, maximize=maximize, **hyper), inputs.size(0), inputs.size(0))
            if ((batch + 1) % DISP_FREQ == 0) and batch != 0:
                display(queue, side, names, epoch)
            if verify and ((batch + 1) % VER_FREQ == 0) and batch != 0:
                with torch.no_grad():
                    kw = dict(testloader_forget=testloader_forget, testloader_remain=testloader_remain, device=device, batch=batch, epoch=epoch,
                              task_i=task_i, forget_acc_before=forget_acc_before, highest_H_mean=highest_H_mean, cfg=cfg, optimizer=optimizer)
                    if testloader_open is not None:
                        kw["testloader_open"] = testloader_open
                    highest_H_mean = evaluate(student, **kw)
                student.train()
            batch += 1

    for i in range(10):
        epoch = superepoch * 15 + i
        sgda_adjust_learning_rate(epoch, cfg, optimizer)
        if i < 5:      # max steps + min steps
            one_pass(data_loader_forget, True, epoch, False)
            one_pass(remain_loader, False, epoch, False)
        else:          # min steps
            one_pass(remain_loader, False, epoch, True)
    forget_q.flush(meters)
    remain_q.flush(meters)
    swa_model.update_parameters(student)
    return (batch, highest_H_mean, losses_CE, losses_total_forget, losses_total_remain, losses_kd_forget, losses_kd_remain, swa_model)
