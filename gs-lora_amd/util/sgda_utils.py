"""The three names of the reference's util/sgda_utils.py, with its signatures, on the HIP path: the step schedule of SCRUB's learning rate
(host arithmetic), DistillKL and param_dist (gslora_hip.kd: libgslora_kd.so, opened on first use)."""
import weakref

from gslora_hip.kd import DistillKL, ParamDist  # noqa: F401  (DistillKL is re-exported under the reference's name)


def adjust_learning_rate(epoch, opt, optimizer):
    """The step schedule of SCRUB's learning rate. k is the number of decay epochs — the entries of opt["lr_decay_epochs"], a sequence or
    the single epoch the driver's config stores — that lie strictly below `epoch`; the rate is opt["sgda_learning_rate"] times
    opt["lr_decay_rate"] to the power k. Before the first decay (k == 0) the optimizer is left as it was built; from then on every param
    group gets the rate. Returns the rate."""
    decay_epochs = opt["lr_decay_epochs"]
    if not hasattr(decay_epochs, "__iter__"):
        decay_epochs = (decay_epochs,)
    k = len([e for e in decay_epochs if e < epoch])
    if k == 0:
        return opt["sgda_learning_rate"]
    rate = opt["sgda_learning_rate"] * opt["lr_decay_rate"] ** k
    for group in optimizer.param_groups:
        group["lr"] = rate
    return rate


_DISTS = weakref.WeakKeyDictionary()      # model -> {id(swa_model): (weak reference to swa_model, ParamDist)}; a ParamDist holds its models weakly


def param_dist(model, swa_model, p):
    """p * sum over zip(model.parameters(), swa_model.parameters()) of the Frobenius norm of the difference, as one autograd node over the
    batched kernels. A ParamDist is built once per (model, swa_model) pair and kept while the model lives; p == 0
    launches nothing."""
    per_model = _DISTS.setdefault(model, {})
    hit = per_model.get(id(swa_model))
    if hit is None or hit[0]() is not swa_model or hit[1].p != float(p):
        hit = (weakref.ref(swa_model), ParamDist(model, swa_model, p))
        per_model[id(swa_model)] = hit
    return hit[1].loss()
