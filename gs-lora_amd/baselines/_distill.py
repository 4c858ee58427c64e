"""The epoch loop the three distillation baselines share (Lwftrain.py, DERtrain.py, FDRtrain.py): in the reference the three loops are one
text with different loss lines. The structure is the reference's: a remain prefetcher that restarts when exhausted, one step per forget
batch, display every DISP_FREQ steps with the meters reset in place, `evaluate` every VER_FREQ steps, the next remain batch drawn at the
end of the step. The loop body is gslora_hip.step.distill_step. Differences that are deliberate, as in SCRUBtrain.py:
  * one deferred host sync per display interval instead of three or four `.item()` per step (meter values are identical);
  * wandb is optional, as in engine_cl.
"""
import torch

from engine_cl import _log, evaluate
from gslora_hip.step import MeterQueue, distill_step
from util.data_prefetcher import data_prefetcher

DISP_FREQ = 5
VER_FREQ = 100


class DistillQueue(MeterQueue):
    """MeterQueue over distill_step's [ce_f, reg, ce_aux, total] packs; every meter is weighted with the forget batch's size, as in the
    reference. A loop names its meters through ORDER ("_unused" entries are not kept)."""
    WEIGHT = ("f", "f", "f", "f")


def run_epoch(student_model, teacher_model, data_loader_cl_forget, remain_loader, criterion, optimizer, device, epoch, batch, meters, queue,
              display, task_i, testloader_forget, testloader_remain, forget_acc_before, highest_H_mean, cfg, testloader_open, *, method, lam,
              lam_aux=0.0, plus=False, check_first_draw=False, step=None):
    """meters: name -> AverageMeter for queue.ORDER; display: (label, meter name) in the order of the reference's print line; step: the
    step function (distill_step; the tests pass a recording stub). -> (batch, highest_H_mean)"""
    step = step or distill_step
    student_model.train()
    teacher_model.eval()

    def draw(prefetcher):      # the reference's "next, and restart when exhausted"
        x, y = prefetcher.next()
        if x is None:
            prefetcher = data_prefetcher(remain_loader, device=device, prefetch=True)
            x, y = prefetcher.next()
        return prefetcher, x, y

    prefetcher_remain = data_prefetcher(remain_loader, device=device, prefetch=True)
    inputs_remain, labels_remain = prefetcher_remain.next()
    if check_first_draw and inputs_remain is None:      # (DERtrain.py:49-51)
        prefetcher_remain = data_prefetcher(remain_loader, device=device, prefetch=True)
        inputs_remain, labels_remain = prefetcher_remain.next()
    for inputs_forget, labels_forget in iter(data_loader_cl_forget):
        inputs_forget, labels_forget = inputs_forget.to(device), labels_forget.to(device)
        extra = {}
        if plus:      # DER++: a second remain batch, drawn inside the step (DERtrain.py:80-86)
            prefetcher_remain, x_n, y_n = draw(prefetcher_remain)
            extra = dict(x_n=x_n, y_n=y_n)
        pack = step(student_model, teacher_model, optimizer, criterion, inputs_forget, labels_forget, inputs_remain, labels_remain, method=method,
                    lam=lam, lam_aux=lam_aux, **extra)
        queue.push(pack, inputs_forget.size(0), inputs_forget.size(0))
        if ((batch + 1) % DISP_FREQ == 0) and batch != 0:
            queue.flush(meters)
            _log({"epoch_loss_{}-{}".format(name[len("losses_"):], task_i): meters[name].avg for _, name in display})
            print("Task {} Epoch {} Batch {}\t".format(task_i, epoch + 1, batch + 1)
                  + "".join("Training {} Loss {:.4f} ({:.4f})\t".format(label, meters[name].val, meters[name].avg) for label, name in display))
            for _, name in display:
                meters[name].reset()
        if ((batch + 1) % VER_FREQ == 0) and batch != 0:
            with torch.no_grad():
                kw = dict(testloader_forget=testloader_forget, testloader_remain=testloader_remain, device=device, batch=batch, epoch=epoch,
                          task_i=task_i, forget_acc_before=forget_acc_before, highest_H_mean=highest_H_mean, cfg=cfg, optimizer=optimizer)
                if testloader_open is not None:
                    kw["testloader_open"] = testloader_open
                highest_H_mean = evaluate(student_model, **kw)
            student_model.train()
        batch += 1
        prefetcher_remain, inputs_remain, labels_remain = draw(prefetcher_remain)
    queue.flush(meters)
    return batch, highest_H_mean
