"""Per-class evaluation on the GPU (csrc/classstat.hip, engine_cl.eval_data_per_class, util.utils.calculate_prototypes):
  (a) gsl_class_stats against torch.max + bincount on the host: integers, so exact — ties, NaN rows and out-of-range labels included;
  (b) gsl_class_embed_sum against a sequential f32 `+=` loop on the host: bit-equal (the same adds in the same order), run to run too;
  (c) both captured in a HIP graph and replayed;
  (d) eval_data_per_class against eval_data (exactly equal: the same integer hit count) and against the real reference's per-class table
      and prototypes (tests/golden/class_stats_small.npz, tools/make_golden_class_stats.py);
  (e) the driver's --per_class record."""
import os

import numpy as np
import pytest
import torch

from oracle import recipe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from gslora_hip import ops
    return ops


def rounded_logits(B, C, seed):
    """Normal draws rounded to one decimal: most rows of 100 or 1000 columns hold their maximum more than once (first-index rule)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, C, generator=g) * 2).mul(10).round().div(10)


def host_stats(logits, labels, C):
    pred = torch.max(logits, 1)[1]
    ok = (labels >= 0) & (labels < C)
    y, p = labels[ok], pred[ok]
    return (torch.bincount(y, minlength=C), torch.bincount(y[p == y], minlength=C), torch.bincount(y * C + p, minlength=C * C).view(C, C),
            int((~ok).sum()))


# ---------------------------------------------------------------------------------------------------------------- (a) class statistics
@pytest.mark.parametrize("C", [7, 100, 1000])
@pytest.mark.parametrize("B", [1, 3, 64, 512, 517])
def test_counts_hits_and_confusion_match_torch(ops, B, C):
    st = ops.ClassStats(C, "cuda", confusion=True)
    want = [torch.zeros(C, dtype=torch.long), torch.zeros(C, dtype=torch.long), torch.zeros(C, C, dtype=torch.long)]
    for s in range(3):      # the counters persist across batches
        lo = rounded_logits(B, C, seed=1000 * s + B + C)
        y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(7 * s + B + C))
        y[::3] = torch.max(lo, 1)[1][::3]      # a third of the rows are hits
        if s == 1:      # a batch whose rows are slices of a wider buffer: the row stride is not C
            wide = torch.full((B, C + 5), 99.0)
            wide[:, :C] = lo
            st.add(wide.cuda()[:, :C], y.cuda())
        else:
            st.add(lo.cuda(), y.cuda())
        for w, h in zip(want, host_stats(lo, y, C)[:3]):
            w += h
    got = st.finish()
    assert got["bad"] == 0 and got["count"].dtype == torch.int64 and got["confusion"].dtype == torch.int32
    assert torch.equal(got["count"], want[0]) and torch.equal(got["hit"], want[1]) and torch.equal(got["confusion"].long(), want[2])
    assert int(want[1].sum()) >= B and int(want[0].sum()) == 3 * B
    acc = 100 * want[1].double() / want[0].double()      # 0 / 0 = NaN for a class without samples, as the kernel writes it
    assert torch.equal(torch.isnan(got["acc"]), want[0] == 0) and torch.equal(got["acc"][want[0] > 0], acc[want[0] > 0])


def test_ties_resolve_to_the_first_index_and_nan_ranks_highest(ops):
    C = 70      # more than one column per lane for some lanes, none for others in the second pass
    nan, inf = float("nan"), float("inf")
    rows = torch.zeros(12, C)
    rows[0, [5, 64, 69]] = 3.0                      # the same maximum in lane 5 twice (columns 5 and 69) and in lane 0's second column
    rows[1, :] = -inf                               # every column -inf: index 0
    rows[2, [68, 3]] = 1.0; rows[2, 40] = nan       # a NaN beats every number
    rows[3, [66, 2, 30]] = nan                      # several NaN: the first
    rows[4, :] = nan
    rows[5, 69] = 1.0                               # the last column
    rows[6, 0] = -0.0; rows[6, 1:] = -1.0; rows[6, 9] = 0.0      # -0 == +0: the first of them
    rows[7, 10] = inf; rows[7, 20] = inf
    rows[8, 63] = 2.0; rows[8, 64] = 2.0            # a tie across the two passes of the lane loop
    rows[9, 1] = nan; rows[9, 0] = inf              # NaN after +inf
    rows[10, :] = 1.0                               # all equal
    rows[11, :] = -1.0; rows[11, 65] = -0.5
    want = torch.max(rows, 1)[1]
    assert want.tolist() == [5, 0, 40, 2, 0, 69, 0, 10, 63, 1, 0, 65]      # torch's own rule, spelled out
    y = want.clone()
    y[[1, 5]] = 7      # two rows that miss
    st = ops.ClassStats(C, "cuda", confusion=True)
    st.add(rows.cuda(), y.cuda())
    got = st.finish()
    cnt, hit, conf, bad = host_stats(rows, y, C)
    assert torch.equal(got["count"], cnt) and torch.equal(got["hit"], hit) and torch.equal(got["confusion"].long(), conf) and got["bad"] == 0
    assert int(got["confusion"][7, 0]) == 1 and int(got["confusion"][7, 69]) == 1 and int(hit.sum()) == 10


def test_an_out_of_range_label_lands_in_bad_and_nowhere_else(ops):
    C, B = 9, 11
    lo = rounded_logits(B, C, seed=5)
    y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(5))
    y[2], y[5], y[10] = C, -1, 2 ** 40
    guard = torch.full((4 * C + 3,), -12345, dtype=torch.long).cuda()      # counters carved out of a guarded buffer
    buf = guard[C + 1:3 * C + 2]      # count [C] | hit [C] | bad [1]
    buf.zero_()
    conf = torch.zeros(C, C, dtype=torch.int32).cuda()
    ops.class_stats(lo.cuda(), y.cuda(), buf[:C], buf[C:2 * C], buf[2 * C:], conf)
    cnt, hit, cm, bad = host_stats(lo, y, C)
    assert bad == 3 and int(buf[2 * C]) == 3
    assert torch.equal(buf[:C].cpu(), cnt) and torch.equal(buf[C:2 * C].cpu(), hit) and torch.equal(conf.cpu().long(), cm)
    assert int(cnt.sum()) == B - 3
    g = guard.cpu()
    assert (g[:C + 1] == -12345).all() and (g[3 * C + 2:] == -12345).all()      # nothing next to the counters was touched
    # the embedding sums skip the same rows
    D = 20
    emb = torch.randn(B, D, generator=torch.Generator().manual_seed(6))
    sums, c2 = torch.zeros(C, D).cuda(), torch.zeros(C + 1, dtype=torch.long).cuda()
    ops.class_embed_sum(emb.cuda(), y.cuda(), sums, c2[:C], c2[C:])
    assert torch.equal(c2[:C].cpu(), cnt) and int(c2[C]) == 3
    ok = (y >= 0) & (y < C)
    assert torch.equal(sums.cpu(), host_embed_sum(torch.zeros(C, D), emb[ok], y[ok]))


# ---------------------------------------------------------------------------------------------------------------- (b) class embedding sums
def host_embed_sum(sums, emb, labels):
    """The reference's accumulation (util/utils.py:540-542): one f32 row add per sample, in sample order."""
    for e, c in zip(emb, labels.tolist()):
        sums[c] += e
    return sums


def embed_batches(B, D, C, n, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        emb = torch.randn(B, D, generator=g)
        y = torch.randint(0, C, (B,), generator=g)
        y[y == C - 1] = 0      # the last class never occurs, class 0 is frequent
        out.append((emb, y))
    return out


def device_embed_sum(ops, batches, C, D, stream=None):
    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        sums, cnt = torch.zeros(C, D, device="cuda"), torch.zeros(C + 1, dtype=torch.long, device="cuda")
        for emb, y in batches:
            ops.class_embed_sum(emb.cuda(), y.cuda(), sums, cnt[:C], cnt[C:])
        _, proto = ops.class_finish(cnt[:C], sums=sums)
        res = sums.cpu(), cnt.cpu(), proto.cpu()
    return res


# B = 1100 crosses the 1024 labels one LDS chunk holds; D = 300 is two column blocks, the second ragged; D = 70 less than one
@pytest.mark.parametrize("B,D,C", [(1, 70, 7), (5, 128, 7), (64, 300, 100), (517, 128, 100), (1100, 70, 7), (130, 512, 1000)])
def test_embed_sum_is_bit_equal_to_the_sequential_host_loop(ops, B, D, C):
    batches = embed_batches(B, D, C, 3, seed=B + D + C)
    want = torch.zeros(C, D)
    for emb, y in batches:
        host_embed_sum(want, emb, y)
    wcnt = sum(torch.bincount(y, minlength=C) for _, y in batches)
    sums, cnt, proto = device_embed_sum(ops, batches, C, D)
    assert torch.equal(cnt[:C], wcnt) and int(cnt[C]) == 0
    assert sums.numpy().tobytes() == want.numpy().tobytes()
    has = wcnt > 0
    assert proto[has].numpy().tobytes() == (want[has] / wcnt[has].float()[:, None]).numpy().tobytes()      # the f32 division of :547
    assert torch.isnan(proto[~has]).all() and int((~has).sum()) >= 1
    # the same accumulation in one batch or in three gives the same bits: the order is the sample order either way
    one = [(torch.cat([e for e, _ in batches]), torch.cat([y for _, y in batches]))]
    sums1, cnt1, _ = device_embed_sum(ops, one, C, D)
    assert sums1.numpy().tobytes() == want.numpy().tobytes() and torch.equal(cnt1, cnt)


def test_embed_sum_two_runs_in_fresh_streams_are_bit_identical(ops):
    B, D, C = 512, 512, 100
    batches = embed_batches(B, D, C, 3, seed=99)
    a = device_embed_sum(ops, batches, C, D, stream=torch.cuda.Stream())
    b = device_embed_sum(ops, batches, C, D, stream=torch.cuda.Stream())
    for x, y in zip(a, b):
        assert x.numpy().tobytes() == y.numpy().tobytes()
    row = torch.zeros(B, D + 3)      # rows taken with their stride
    row[:, :D] = batches[0][0]
    s1, c1 = torch.zeros(C, D).cuda(), torch.zeros(C + 1, dtype=torch.long).cuda()
    ops.class_embed_sum(row.cuda()[:, :D], batches[0][1].cuda(), s1, c1[:C], c1[C:])
    assert s1.cpu().numpy().tobytes() == host_embed_sum(torch.zeros(C, D), *batches[0]).numpy().tobytes()


# ---------------------------------------------------------------------------------------------------------------- (c) HIP graph
def test_both_kernels_replay_from_a_hip_graph(ops):
    B, C, D = 37, 23, 96
    lo_s, emb_s, y_s = torch.zeros(B, C).cuda(), torch.zeros(B, D).cuda(), torch.zeros(B, dtype=torch.long).cuda()
    st = ops.ClassStats(C, "cuda", confusion=True)
    sums, cnt = torch.zeros(C, D).cuda(), torch.zeros(C + 1, dtype=torch.long).cuda()
    proto = torch.empty(C, D).cuda()
    warm = ops.ClassStats(C, "cuda", confusion=True)      # first launches load the code object: not inside a capture
    warm.add(lo_s, y_s)
    ops.class_embed_sum(emb_s, y_s, torch.zeros(C, D).cuda(), warm.count.clone(), warm.bad.clone())
    warm.finish()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):      # nothing in these calls allocates or synchronises
        st.add(lo_s, y_s)
        ops.class_embed_sum(emb_s, y_s, sums, cnt[:C], cnt[C:])
        ops.class_finish(st.count, st.hit, sums=sums, acc=st.acc, proto=proto)
    assert int(st.buf.abs().sum()) == 0 and int(cnt.sum()) == 0      # capturing ran nothing
    eager = ops.ClassStats(C, "cuda", confusion=True)
    e_sums, e_cnt = torch.zeros(C, D).cuda(), torch.zeros(C + 1, dtype=torch.long).cuda()
    for s in range(3):
        lo = rounded_logits(B, C, seed=40 + s).cuda()
        emb = torch.randn(B, D, generator=torch.Generator().manual_seed(50 + s)).cuda()
        y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(60 + s)).cuda()
        lo_s.copy_(lo), emb_s.copy_(emb), y_s.copy_(y)
        graph.replay()
        eager.add(lo, y)
        ops.class_embed_sum(emb, y, e_sums, e_cnt[:C], e_cnt[C:])
    torch.cuda.synchronize()
    e_acc, e_proto = ops.class_finish(eager.count, eager.hit, sums=e_sums)
    assert torch.equal(st.buf[:2 * C + 1], eager.buf[:2 * C + 1]) and torch.equal(st.confusion, eager.confusion) and int(st.count.sum()) == 3 * B
    assert torch.equal(sums, e_sums) and torch.equal(cnt, e_cnt)
    assert st.acc.cpu().numpy().tobytes() == e_acc.cpu().numpy().tobytes() and proto.cpu().numpy().tobytes() == e_proto.cpu().numpy().tobytes()


# ---------------------------------------------------------------------------------------------------------------- (d) the Python surface
def loader_of(cfg, n, batch, seed, num_class=None):
    from torch.utils.data import DataLoader, TensorDataset
    x = torch.tensor(recipe.make_images(cfg, n, seed=seed, tag="pc_x"))
    y = torch.tensor(recipe.make_labels(dict(cfg, num_class=num_class or cfg["num_class"]), n, seed=seed, tag="pc_y"))
    return DataLoader(TensorDataset(x, y), batch_size=batch, shuffle=False), y


def model_state(net):
    return dict(training=[m.training for m in net.modules()], dtype=getattr(net, "compute_dtype", None),
                merged=[getattr(m, "merged", None) for m in net.modules()])


def _vit_face(dtype):
    from test_hip_heads import build
    cfg = recipe.cfg_small2()
    return build(cfg, "Softmax", dtype), cfg, cfg["num_class"]


def _vits_face(dtype):
    from test_hip_vits import build
    cfg = recipe.cfg_small2()
    return build(cfg, "CosFace", dtype=dtype), cfg, cfg["num_class"]


def _modified_vit(dtype):
    from test_hip_vitb import build_full
    cfg = recipe.cfg_vitb_small2()
    return build_full(cfg, dtype), cfg, cfg["num_class"]


@pytest.mark.parametrize("make,dtype", [(_vit_face, "fp32"), (_vit_face, "bf16"), (_vits_face, "fp32"), (_modified_vit, "fp32")])
def test_accuracy_equals_eval_data_exactly_and_the_model_is_left_as_eval_data_leaves_it(make, dtype):
    import engine
    import engine_cl
    model, cfg, C = make(dtype)
    loader, y = loader_of(cfg, 23, 5, seed=77, num_class=C)      # 4 full batches and a ragged one of 3
    model.train()
    want = engine_cl.eval_data(model, loader, "cuda", "plain")
    after_eval_data = model_state(model)
    model.train()
    got = engine_cl.eval_data_per_class(model, loader, "cuda", "per-class", num_classes=C, confusion=True)
    assert model_state(model) == after_eval_data and not model.training      # eval mode stays, as after eval_data; the compute dtype is back
    assert got["accuracy"] == want
    tot, cor, conf = got["class_total"], got["class_correct"], got["confusion"]
    assert torch.equal(tot, torch.bincount(y, minlength=C)) and int(tot.sum()) == 23 and (cor <= tot).all()
    assert got["accuracy"] == 100 * int(cor.sum()) / 23
    assert torch.equal(conf.sum(1).long(), tot) and torch.equal(conf.diagonal().long(), cor) and tuple(conf.shape) == (C, C)
    acc = got["class_accuracy"]
    assert acc.dtype == torch.float64 and torch.equal(torch.isnan(acc), tot == 0)
    assert acc[tot > 0].tolist() == [100 * c / t for c, t in zip(cor[tot > 0].tolist(), tot[tot > 0].tolist())]
    assert "confusion" not in engine_cl.eval_data_per_class(model, loader, "cuda", "per-class")
    with pytest.raises(ValueError, match="num_classes"):
        engine_cl.eval_data_per_class(model, loader, "cuda", "per-class", num_classes=C + 1)
    # the single-task engine evaluates a copy: mode, merge state and the un-merged weights come back
    model.train()
    before = model_state(model)
    w0 = {n: p.detach().clone() for n, p in model.state_dict().items()}
    got1 = engine.eval_data_per_class(model, loader, "cuda", "single", confusion=True)
    assert model_state(model) == before and model.training
    assert all(torch.equal(w0[n], p) for n, p in model.state_dict().items())
    assert got1["accuracy"] == engine.eval_data(model, loader, "cuda", "single") == want
    assert torch.equal(got1["class_correct"], cor) and torch.equal(got1["confusion"], conf)


def test_a_label_outside_the_classes_is_an_error():
    import engine_cl
    from torch.utils.data import DataLoader, TensorDataset
    model, cfg, C = _vit_face("fp32")
    x = torch.tensor(recipe.make_images(cfg, 4, seed=3, tag="pc_x"))
    with pytest.raises(ValueError, match="outside"):
        engine_cl.eval_data_per_class(model, DataLoader(TensorDataset(x, torch.tensor([0, 1, C, 2])), batch_size=4), "cuda", "bad")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "class_stats_small.npz"))


def test_per_class_table_matches_the_reference(golden, tmp_path):
    """(a) of tools/make_golden_class_stats.py: test/test_own.py:99-143 of the real reference on 48 seeded images, batches of 6."""
    import engine_cl
    from torch.utils.data import DataLoader, TensorDataset
    from util.utils import write_class_accuracy
    model, cfg, C = _vit_face("fp32")
    x = torch.tensor(recipe.make_images(cfg, 48, seed=500, tag="cs_x"))      # = stats_inputs() of the generator
    y = torch.tensor(golden["stats_labels"])
    for batch in (int(golden["stats_batch"]), 7):      # the reference's batch size, and one that leaves a ragged tail (48 = 6 * 7 + 6)
        got = engine_cl.eval_data_per_class(model, DataLoader(TensorDataset(x, y), batch_size=batch), "cuda", "golden")
        assert got["class_total"].tolist() == golden["stats_total"].tolist()
        assert got["class_correct"].tolist() == golden["stats_correct"].tolist()
        assert got["accuracy"] == float(golden["stats_accuracy"])
        path = str(tmp_path / "class_accuracy.txt")
        write_class_accuracy(path, got["class_correct"], got["class_total"])
        assert open(path).read().split("\n")[:-1] == golden["stats_lines"].tolist()
        assert ["%4.4f %%" % a for a in got["class_accuracy"].tolist()] == golden["stats_lines"].tolist()


def test_prototypes_match_the_reference(golden):
    """(b): the reference's calculate_prototypes on 23 images in batches of 5, at the bar of test_hip_model.test_prototypes_match_reference."""
    from util.utils import calculate_prototypes
    model, cfg, C = _vit_face("fp32")
    model.train()
    x = torch.tensor(recipe.make_images(cfg, 23, seed=600, tag="cp_x"))      # = proto_inputs() of the generator
    ds = torch.utils.data.TensorDataset(x, torch.tensor(golden["proto_labels"]))
    protos = calculate_prototypes(model, ds, batch_size=int(golden["proto_batch"]), device="cuda")
    assert sorted(protos) == golden["proto_keys"].tolist() and int(golden["proto_absent"]) not in protos
    assert all(v.device.type == "cpu" and v.dtype == torch.float32 and tuple(v.shape) == (cfg["dim"],) for v in protos.values())
    got = np.stack([protos[k].numpy() for k in sorted(protos)])
    assert np.abs(got - golden["proto_vals"]).max() < 1e-4
    assert not model.training      # the reference leaves the model in eval() too
    # a second run gives the same bits: no sum depends on an arrival order
    again = calculate_prototypes(model, ds, batch_size=int(golden["proto_batch"]), device="cuda")
    assert all(torch.equal(protos[k], again[k]) for k in protos)


# ---------------------------------------------------------------------------------------------------------------- (e) the driver
PARENT_RECORD_KEYS = {"task", "steps", "lrs", "hypers", "norms", "total_loss", "forget_before", "forget_after", "remain_before", "remain_after",
                      "ema_acc", "ema_accs", "forget_cls"}


def test_driver_per_class_record(tmp_path, monkeypatch):
    import driver_cl
    argv = ["--small", "--num_class", "10", "--num_tasks", "1", "--per_forget_cls", "3", "--epochs", "1", "--batch_size", "16",
            "--samples_per_class", "4", "--dtype", "fp32", "--dropout", "0.0"]
    off, _, _ = driver_cl.main(argv + ["--outdir", str(tmp_path / "off")])
    assert set(off[0]) == PARENT_RECORD_KEYS      # without the flag the record is the parent commit's
    run_tasks = driver_cl.run_tasks      # the keyword of run_tasks itself; `--per_class` sets args.per_class, which it defaults to
    monkeypatch.setattr(driver_cl, "run_tasks", lambda *a, **kw: run_tasks(*a, per_class=True, **kw))
    on, _, _ = driver_cl.main(argv + ["--outdir", str(tmp_path / "on")])
    for rep in (on,):
        rec = rep[0]
        assert set(rec) == PARENT_RECORD_KEYS | {"per_class"}
        assert {k: rec[k] for k in PARENT_RECORD_KEYS} == off[0]      # the per-class pass changes nothing else of the run
        pc, forget = rec["per_class"], rec["forget_cls"]
        assert sorted(pc["forget"]) == sorted(forget) and sorted(pc["remain"]) == sorted(set(range(10)) - set(forget))
        # two test images per class: the per-class accuracies average to the aggregate eval_data reports
        assert abs(sum(pc["forget"].values()) / 3 - rec["forget_after"]) < 1e-9 and abs(sum(pc["remain"].values()) / 7 - rec["remain_after"]) < 1e-9
        assert sorted(pc["forget_top3"]) == sorted(forget)
        for c, top in pc["forget_top3"].items():
            assert 1 <= len(top) <= 3 and sum(n for _, n in top) <= 2 and all(0 <= p < 10 and n >= 1 for p, n in top)
            assert [n for _, n in top] == sorted((n for _, n in top), reverse=True)
            hit = dict(top).get(c, 0)
            assert hit == round(pc["forget"][c] * 2 / 100)
