"""engine_reg — the epoch loop of the regularisation baselines (L2 / EWC / MAS), MI355X-native counterpart of the reference's
`engine_cl.train_one_epoch_regularzation` (engine_cl.py:463-568): same name, same 19 parameters, same 5-tuple. Import it from HERE:

    from engine_reg import train_one_epoch_regularzation

`engine_cl.train_one_epoch_regularzation` of this package keeps its name only and raises (it is pinned that way: a caller that reaches it
without the baselines' set-up — a model built with lora_rank = 0, the --only_ffn trainability rule — gets a refusal, not a silent
full-weight run). The loop body is gslora_hip.step.ffn_reg_step with the terms prepared once per call as a gslora_hip.reg.RegTerms: the
regulariser costs two launches forward and one backward whatever the number of terms. Differences that are deliberate:
  * one deferred host sync per display interval instead of three `.item()` per step (meter values are identical);
  * wandb is optional, as in engine_cl.
"""
import torch

import util.utils as util
from engine_cl import DISP_FREQ, VER_FREQ, _log, evaluate
from gslora_hip.step import MeterQueue, ffn_reg_step


class RegMeterQueue(MeterQueue):
    """MeterQueue over ffn_reg_step's [CE, regularisation, total, prec1 %] packs (engine_cl.py:497-508: all weighted with the batch size;
    the reference keeps no accuracy meter in this loop)."""
    ORDER = ("losses_CE", "losses_regularization", "losses_total", "top1")
    WEIGHT = ("r", "r", "r", "r")


def train_one_epoch_regularzation(model: torch.nn.Module, criterion: torch.nn.Module, data_loader_cl_forget, optimizer, device, epoch: int,
                                  batch: int, reg_lambda: float, regularization_terms: dict, losses_CE, losses_regularization, losses_total,
                                  task_i: str, testloader_forget, testloader_remain, forget_acc_before: float, highest_H_mean: float,
                                  cfg: dict, testloader_open=None):
    """One pass over the loader: forward, cross-entropy, get_reg_loss, zero_grad, backward, step (engine_cl.py:490-512), the display every
    DISP_FREQ steps (:515-547), evaluate every VER_FREQ steps (:548-564). Returns (batch, highest_H_mean, losses_CE, losses_regularization,
    losses_total)."""
    from gslora_hip.reg import RegTerms
    model.train()
    criterion.train()
    terms = RegTerms(model, regularization_terms, reg_lambda) if regularization_terms is not None else None
    meters = dict(losses_CE=losses_CE, losses_regularization=losses_regularization, losses_total=losses_total)
    queue = RegMeterQueue()
    for inputs_forget, labels_forget in iter(data_loader_cl_forget):
        inputs_forget, labels_forget = inputs_forget.to(device), labels_forget.to(device)
        pack = ffn_reg_step(model, optimizer, criterion, inputs_forget, labels_forget, regularization_terms=terms, reg_lambda=reg_lambda)
        queue.push(pack, inputs_forget.size(0), inputs_forget.size(0))

        if ((batch + 1) % DISP_FREQ == 0) and batch != 0:
            queue.flush(meters)
            m = meters
            _log({"epoch_loss_CE-{}".format(task_i): m["losses_CE"].avg,
                  "epoch_loss_regularization-{}".format(task_i): m["losses_regularization"].avg,
                  "epoch_loss_total-{}".format(task_i): m["losses_total"].avg})
            print("Task {} Epoch {} Batch {}\t"
                  "Training CE Loss {:.4f} ({:.4f})\tTraining regularization Loss {:.4f} ({:.4f})\tTraining total Loss {:.4f} ({:.4f})".format(
                      task_i, epoch + 1, batch + 1, m["losses_CE"].val, m["losses_CE"].avg, m["losses_regularization"].val,
                      m["losses_regularization"].avg, m["losses_total"].val, m["losses_total"].avg))
            for k in meters:      # the reference re-binds fresh meters after each display (:544-547)
                meters[k] = util.AverageMeter()

        if ((batch + 1) % VER_FREQ == 0) and batch != 0:
            with torch.no_grad():
                kw = dict(testloader_forget=testloader_forget, testloader_remain=testloader_remain, device=device, batch=batch, epoch=epoch,
                          task_i=task_i, forget_acc_before=forget_acc_before, highest_H_mean=highest_H_mean, cfg=cfg, optimizer=optimizer)
                if testloader_open is not None:
                    kw["testloader_open"] = testloader_open
                highest_H_mean = evaluate(model, **kw)
            model.train()

        batch += 1

    queue.flush(meters)
    return batch, highest_H_mean, meters["losses_CE"], meters["losses_regularization"], meters["losses_total"]
