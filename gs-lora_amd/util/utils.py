"""Step helpers of the reference's util/utils.py that sit on the GS-LoRA path
(AverageMeter :316-332, train_accuracy :354-368, count_trainable_parameters :423-425,
reinitialize_lora_parameters :428-441, calculate_prototypes :502-549, replace_ffn_with_lora :552-577,
modify_head :580-621, resume_head :623-636, create_few_shot_dataset :457-499, get_unique_classes :444-454) and its face verification
(perform_val :167-230, buffer_val :298-314), backed by the HIP model and the HIP metric kernels (util/verification.py);
write_class_accuracy writes the per-class accuracy file of test/test_own.py:140-143.
Data plumbing (load_bin / get_val_pair: mxnet, bcolz) and perform_val_deit are out of scope."""
import copy
import datetime
import math
import os
import random
from collections import defaultdict

import torch

from image_iter import CustomSubset  # noqa: E402,F401  (defined where the reference defines it: image_iter.py:124-137; util/utils.py:30 imports it)
import torch.nn as nn


class AverageMeter(object):
    """val / avg / sum / count running mean — same update arithmetic as the reference."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def train_accuracy(output, target, topk=(1,)):
    """precision@k in percent. topk=(1,) (all the engines ask for): the 0-dim tensor of the fused CE / top-1 launch. Any other tuple: a
    list with one 0-dim tensor per k, in the order given, from one HIP launch (gsl_topk_hits: a row is a hit when fewer than k logits are
    strictly greater than its label's — output.topk(maxk) wherever the k-th place is not tied). The reference computes the same list and
    returns its first entry alone (:368); the first entry here is that value."""
    topk = tuple(int(k) for k in topk)
    from gslora_hip import ops
    if topk == (1,):
        out = ops.ce_fwd(output.detach().float().contiguous(), target.to(output.device, torch.int64).contiguous())
        return out[1] * (100.0 / target.size(0))
    if not topk or min(topk) < 1 or max(topk) > output.size(1):
        raise ValueError(f"train_accuracy: every k of topk must lie in [1, {output.size(1)}] (the number of classes), got {topk}")
    hits = ops.topk_hits(output.detach().float().contiguous(), target.to(output.device, torch.int64).contiguous(), topk)
    pct = hits.to(torch.float32) * (100.0 / target.size(0))
    return [pct[i] for i in range(len(topk))]


def count_trainable_parameters(model):
    return sum(p.numel() for p in model.parameters() if p.requires_grad)


def reinitialize_lora_parameters(model):
    """Fresh adapters for the next task: A ~ kaiming_uniform(a=sqrt(50)), B = 0 (in place, so the
    parameters stay views of the flat LoRA bucket)."""
    with torch.no_grad():
        for name, param in model.named_parameters():
            if "lora" in name:
                if not isinstance(param, nn.Parameter):
                    raise ValueError(f"Parameter {name} is not an instance of nn.Parameter.")
                if "lora_A" in name:
                    nn.init.kaiming_uniform_(param, a=math.sqrt(50))
                elif "lora_B" in name:
                    nn.init.zeros_(param)


def calculate_prototypes(backbone, dataset, batch_size=32, device="cuda", aug_num=0):
    """Per-class mean embedding in eval (merged-LoRA) mode; leaves the model in eval() like the
    reference does. Class sums are accumulated on the device, one gsl_class_embed_sum launch per batch: each class adds its embeddings
    one by one in sample order, the reference's `embeds_sum[label] += embed` (:540-542), so the f32 sums do not depend on the batch size
    or on the run. The result dict holds CPU tensors, for the classes that occur, as before."""
    from torch.utils.data import ConcatDataset, DataLoader
    from gslora_hip import ops
    backbone.eval()
    backbone.to(device)
    if aug_num != 0:
        # GS-LoRA++ prototype augmentation (reference :506-523): the data set's transform is REPLACED by RandAugment(num_ops=2,
        # magnitude=aug_num) + ToTensor and the set is visited 20 times; the prototypes are the class means over all 20 passes.
        # torchvision supplies the augmentation itself (host-side PIL work, outside the GPU hot path); without it there is nothing to run.
        try:
            import torchvision.transforms as transforms
        except Exception as exc:      # pragma: no cover
            raise RuntimeError("calculate_prototypes(aug_num > 0) needs torchvision.transforms (RandAugment), as in the reference") from exc
        transform = transforms.Compose([transforms.RandAugment(num_ops=2, magnitude=aug_num), transforms.ToTensor()])
        dataset.transform = transform
        dataset = ConcatDataset([dataset] * 20)
        dataset.transform = transform
    loader = DataLoader(dataset, batch_size=batch_size, shuffle=False)
    sums = counts = None
    with torch.no_grad():
        for images, labels in loader:
            images, labels = images.to(device), labels.to(device).long()
            _, emb = backbone(images, labels)
            if sums is None:
                head = getattr(backbone, "loss", None)          # ViT_face: CosFace head; ModifiedViT: torchvision's heads.head
                if head is not None and hasattr(head, "weight"):
                    ncls = head.weight.shape[0]
                elif hasattr(backbone, "heads"):
                    ncls = backbone.heads.head.out_features
                else:
                    ncls = int(labels.max().item()) + 1
                sums = torch.zeros(ncls, emb.shape[1], device=emb.device)
                counts = torch.zeros(ncls + 1, device=emb.device, dtype=torch.int64)      # [ncls] class counts | labels outside [0, ncls)
            ops.class_embed_sum(emb.float(), labels.contiguous(), sums, counts[:ncls], counts[ncls:])
    if sums is None:
        return {}
    protos = ops.class_finish(counts[:ncls], sums=sums)[1].cpu()      # sums / counts, the f32 division of :547
    counts = counts.cpu()
    if int(counts[ncls]):
        raise ValueError(f"calculate_prototypes: {int(counts[ncls])} labels lie outside [0, {ncls}), the classes of the model's head")
    return {int(c): protos[c] for c in torch.nonzero(counts[:ncls]).flatten().tolist()}


def write_class_accuracy(path, class_correct, class_total):
    """The reference's per-class accuracy file (test/test_own.py:140-143, `class_accuracy40.txt`): one line "%4.4f %%" of
    100 * correct / total per class, in class order. class_correct / class_total: sequences or tensors of one length (the `class_correct`
    and `class_total` of eval_data_per_class). A class without samples, where the reference divides by zero, is written as the format renders NaN (" nan %")."""
    correct, total = [float(v) for v in class_correct], [float(v) for v in class_total]
    if len(correct) != len(total):
        raise ValueError(f"write_class_accuracy: {len(correct)} corrects for {len(total)} totals")
    with open(path, "w") as f:
        for c, t in zip(correct, total):
            f.write("%4.4f %%" % (100 * c / t if t else float("nan")))
            f.write("\n")


def _eval_dtype_of(net):
    """The compute dtype evaluation switches to (None: stay in the model's own), chosen as engine_cl.eval_data chooses it."""
    import engine_cl
    if engine_cl.EVAL_DTYPE in engine_cl._EVAL_SAME or not hasattr(net, "set_compute_dtype"):
        return None
    return engine_cl.EVAL_DTYPE


def _compute_mode_of(net):
    """What set_compute_dtype takes to bring `net` back to its current mode after an evaluation in another one: the mode's name ('fp16' | 'bf16' |
    'fp32' | 'fp32x3') where the model has one — its torch dtype cannot tell 'fp32x3' from 'fp32' — else the torch dtype (None: no switch)."""
    return getattr(net, "compute_mode", None) or getattr(net, "compute_dtype", None)


def pair_embeddings(device, embedding_size, batch_size, backbone, data_set):
    """The embedding pass of perform_val (reference :187-203): data_set = [images, flipped images], each [2P, C, H, W] (float, or uint8
    bytes for a model that was given set_input_norm). Batches of batch_size with the ragged tail; the original and the flipped batch of
    the same indices go through ONE forward as two parts. Returns (e0, e1), f32 [2P, embedding_size] on the device. The model must be
    in eval mode already; no mode or dtype is changed here."""
    if len(data_set) != 2 or len(data_set[0]) != len(data_set[1]):
        raise ValueError("perform_val: data_set is [images, flipped images] of one length")
    n = len(data_set[0])
    e = [torch.empty(n, embedding_size, device=device, dtype=torch.float32) for _ in range(2)]
    as_parts = getattr(backbone, "accepts_batch_tuple", False)
    with torch.no_grad():
        idx = 0
        while idx < n:      # full batches, then the ragged tail (:193-202)
            stop = min(idx + batch_size, n)
            parts = [torch.as_tensor(c[idx:stop]).to(device) for c in data_set]
            outs = backbone(tuple(parts)) if as_parts else [backbone(t) for t in parts]
            if as_parts:
                outs = outs[-1] if isinstance(outs, (tuple, list)) else outs      # ModifiedViT returns (logits, cls embeddings)
                outs = [outs[:stop - idx], outs[stop - idx:]]
            else:
                outs = [o[-1] if isinstance(o, (tuple, list)) else o for o in outs]
            for dst, o in zip(e, outs):
                if o.shape != (stop - idx, embedding_size):
                    raise ValueError(f"perform_val: the backbone returned {tuple(o.shape)} for {stop - idx} images, embedding_size is {embedding_size}")
                dst[idx:stop] = o
            idx = stop
    return e[0], e[1]


def perform_val(multi_gpu, device, embedding_size, batch_size, backbone, data_set, issame, nrof_folds=10):
    """Face verification on a pair set (LFW etc.; reference :167-230): embeddings of the images and of their flipped copies, summed and
    normalised, squared distance per pair, nrof_folds-fold threshold selection. Embeddings stay on the device; the metric runs in the HIP
    kernels of util/verification.py with one host read at the end.

    :return: (accuracy.mean(), accuracy.std(), xnorm, best_thresholds.mean(), roc) as the reference, except the fifth element: the ROC
        itself, a float32 CPU tensor [2, 400] = (fpr, tpr) over the thresholds np.arange(0, 4, 0.01), not a matplotlib JPEG of it.

    The evaluation dtype is engine_cl.eval_data's (GSLORA_EVAL_DTYPE, f32 by default). Unlike the reference, which leaves the model in
    eval(), the model's train / eval mode (and with it the LoRA merge state) and its compute dtype are restored before returning."""
    import numpy as np
    from gslora_hip import ops
    from util import verification
    if multi_gpu:
        backbone = backbone.module      # unpackage model from DataParallel
    backbone = backbone.to(device)
    verification.fold_bounds(len(issame), nrof_folds)      # argument errors before any GPU work
    was_training = backbone.training
    eval_dt, own_dt = _eval_dtype_of(backbone), _compute_mode_of(backbone)
    backbone.eval()
    if eval_dt:
        backbone.set_compute_dtype(eval_dt)
    try:
        e0, e1 = pair_embeddings(device, embedding_size, batch_size, backbone, data_set)
    finally:
        if eval_dt:
            backbone.set_compute_dtype(own_dt)
        backbone.train(was_training)
    dist, xnorm, _ = ops.verif_pair_dist(e0, e1)
    print("embeddings shape", tuple(e0.shape))
    tpr, fpr, accuracy, best_thresholds, xn = verification.roc_from_dist(verification.THRESHOLDS, dist[:len(issame)], issame, nrof_folds, xnorm)
    roc = torch.from_numpy(np.stack([fpr, tpr]).astype(np.float32))
    return accuracy.mean(), accuracy.std(), xn, best_thresholds.mean(), roc


def buffer_val(db_name, acc, std, xnorm, best_threshold, roc_curve_tensor, batch):
    """Log one perform_val result (reference :298-314 sends the four scalars to wandb; here they go to wandb when it is importable and a
    run is active, and are returned either way)."""
    rec = {"{}_Accuracy".format(db_name): acc, "{}_Std".format(db_name): std, "{}_XNorm".format(db_name): xnorm,
           "{}_Best_Threshold".format(db_name): best_threshold}
    try:
        import wandb
        if getattr(wandb, "run", None) is not None:
            wandb.log(rec, step=batch)
    except ImportError:
        pass
    return rec


def get_unique_classes(subset, original_dataset):
    """(class names, number of classes) of a subset (reference :444-454)."""
    return subset.classes, len(subset.classes)


def create_few_shot_dataset(dataset, n_shot, seed=None):
    """n_shot random samples per class, shuffled — the same `random` call sequence as the reference (:457-499), so a given seed
    selects the same indices (tests/golden/host_kats.npz)."""
    if seed is not None:
        random.seed(seed)
    if not hasattr(dataset, "targets"):
        raise AttributeError("The dataset object needs to have a 'targets' attribute to access the labels.")
    targets = dataset.targets
    if isinstance(targets, torch.Tensor):
        targets = targets.tolist()
    by_class = defaultdict(list)
    for idx, label in enumerate(targets):
        by_class[label].append(idx)
    picked = []
    for cls, indices in by_class.items():
        if len(indices) < n_shot:
            raise ValueError(f"Class {cls} has fewer samples than {n_shot}.")
        picked.extend(random.sample(indices, n_shot))
    random.shuffle(picked)
    return CustomSubset(dataset, picked)


def get_time():
    return (str(datetime.datetime.now())[:-10]).replace(" ", "-").replace(":", "-")


# ---- ViT-B/16 ImageNet100 model surgery --------------------------------------------------------------------------
HEAD_CACHE = "results/original_VIT_head/classifier.pth"     # same relative path as the reference (:593-597, :628)


def replace_ffn_with_lora(model, rank=8):
    """Swap the two nn.Linear of every `.mlp` for loralib.Linear(r=rank) (reference :552-577). As in the reference the new
    layers are freshly initialised — the frozen FFN weights come from the checkpoint the driver loads afterwards
    (train_own_forget_cl.py:250-262)."""
    import loralib as lora
    from gslora_hip.ops import check_lora_rank
    check_lora_rank(type(model).__name__, rank)      # refused here, where the adapters are attached, not in the first forward
    for _, module in list(model.named_modules()):
        if hasattr(module, "mlp"):
            ffn = module.mlp
            for ffn_name, ffn_layer in list(ffn.named_children()):
                if isinstance(ffn_layer, nn.Linear) and not isinstance(ffn_layer, lora.Linear):
                    new = lora.Linear(ffn_layer.in_features, ffn_layer.out_features, r=rank)
                    setattr(ffn, ffn_name, new.to(ffn_layer.weight.device))
    return model


def modify_head(model_ori, current_id_to_original_id, device):
    """Deep-copied model whose classifier keeps only the rows of the listed original class ids, in dict order
    (reference :580-621). The untouched 1000-way head is saved once to HEAD_CACHE for resume_head."""
    model = copy.deepcopy(model_ori)
    old = model.heads.head
    old_w, old_b = old.weight.data, old.bias.data
    if not os.path.exists(HEAD_CACHE):
        os.makedirs(os.path.dirname(HEAD_CACHE), exist_ok=True)
        torch.save(old.state_dict(), HEAD_CACHE)
    ids = torch.tensor([int(i) for i in current_id_to_original_id.values()], dtype=torch.long, device=old_w.device)
    new = nn.Linear(old.in_features, len(current_id_to_original_id))
    new.weight.data = old_w.index_select(0, ids).clone()
    new.bias.data = old_b.index_select(0, ids).clone()
    model.heads.head = new
    return model.to(device)


def resume_head(model, device):
    """Deep-copied model with the original 1000-way ImageNet head restored from HEAD_CACHE (reference :623-636)."""
    model = copy.deepcopy(model)
    sd = torch.load(HEAD_CACHE)
    new = nn.Linear(sd["weight"].shape[1], sd["weight"].shape[0])
    new.weight.data = sd["weight"].data
    new.bias.data = sd["bias"].data
    model.heads.head = new
    return model.to(device)
