"""GPU: the training driver end to end on a tiny synthetic dataset: DataLoader + collate_train -> train steps ->
eval_epoch after every epoch -> best checkpoint -> reload.  Captions are noisy copies of a clip of their video
(through a fixed random projection), so the model can learn: SumR must improve and the loss must fall."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class TinySet(torch.utils.data.Dataset):
    def __init__(self, n=24, dv=256, dq=128, seed=0, caps=lambda i: 2):
        g = torch.Generator().manual_seed(seed)
        proj = torch.randn(dv, dq, generator=g) / dv ** 0.5
        tproj_v = torch.randn(dv, 512, generator=g) / dv ** 0.5
        self.items = []
        for i in range(n):
            L = int(torch.randint(4, 13, (1,), generator=g))
            v = torch.nn.functional.normalize(torch.randn(L, dv, generator=g), dim=-1)
            caps_, tcaps = [], []
            for c in range(caps(i)):
                l = int(torch.randint(0, L, (1,), generator=g))
                w = v[l] @ proj
                words = torch.nn.functional.normalize(w.unsqueeze(0) + 0.3 * torch.randn(5 + c, dq, generator=g), dim=-1)
                caps_.append(words)
                tcaps.append((v[l] @ tproj_v).unsqueeze(0) * 3.0)
            self.items.append((v, caps_, v @ tproj_v * 3.0, tcaps, i, [f"v{i}#{c}" for c in range(len(caps_))], f"v{i}"))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]

    def videos(self):
        return [(it[0], it[4], it[6]) for it in self.items]

    def texts(self):
        out = []
        for it in self.items:
            for c, cap in enumerate(it[1]):
                out.append((cap, len(out), it[5][c]))
        return out


class L(torch.utils.data.Dataset):
    def __init__(self, x): self.x = x
    def __len__(self): return len(self.x)
    def __getitem__(self, i): return self.x[i]


def test_train_loop_learns_and_checkpoints(tmp_path):
    from dldkd_amd.model import DLDKD
    from dldkd_amd import train as T
    ds = TinySet()
    cfg = types.SimpleNamespace(visual_input_size=256, query_input_size=128, inheritance_hidden=384, exploration_hidden=384,
                                max_ctx_l=128, max_desc_l=30, input_drop=0.1, drop=0.1, n_heads=4, initializer_range=0.02,
                                margin=0.1, use_hard_negative=False, hard_pool_size=5, label_style="soft")
    opt = types.SimpleNamespace(double_branch=True, kl_intra_weight=0.1, inher_nce_weight=0.04, explore_nce_weight=0.04,
                                collection="tiny", alpha=0.8, belta=0.8, device=torch.device(DEV), bsz=8, pin_memory=False,
                                num_workers=0, lr=1e-3, wd=0.01, lr_warmup_proportion=0.05, n_epoch=6, max_es_cnt=10,
                                hard_negative_start_epoch=0, hard_pool_size=5, distill_loss_decay="exp", exponential_k=0.95,
                                selfDistil_sigmoid_k=800, alpha_decay="sigmoid", belta_decay="sigmoid", grad_clip=-1,
                                eval_context_bsz=16, eval_query_bsz=50, eval_untrained=True,
                                ckpt_filepath=str(tmp_path / "model.ckpt"))
    torch.manual_seed(0)
    m = DLDKD(cfg, opt)
    hist = T.train(m, ds, L(ds.videos()), L(ds.texts()), opt)
    assert hist[0][0] == -1 and len(hist) == 7                     # eval_untrained epoch + 6 epochs
    sumr = [h[2] for h in hist]
    losses = [h[1]["loss_overall"] for h in hist[1:]]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert max(sumr[1:]) > sumr[0] + 20, sumr                      # it learned to retrieve
    assert m.weight == pytest.approx(0.95 ** 5) and m.config.use_hard_negative is True
    m2, ep = T.load_checkpoint(opt.ckpt_filepath, opt)
    assert 0 <= ep <= 5
    with torch.no_grad():
        from dldkd_amd.eval import eval_epoch
        assert eval_epoch(m2.to(DEV), L(ds.videos()), L(ds.texts()), opt) == pytest.approx(max(sumr))


def _fit(precision, tmp_path, force_ddp=False, train_precision=None, ds=None):
    from dldkd_amd.model import DLDKD
    from dldkd_amd import train as T, ops
    ds = ds if ds is not None else TinySet()
    cfg = types.SimpleNamespace(visual_input_size=256, query_input_size=128, inheritance_hidden=384, exploration_hidden=384,
                                max_ctx_l=128, max_desc_l=30, input_drop=0.1, drop=0.1, n_heads=4, initializer_range=0.02,
                                margin=0.1, use_hard_negative=False, hard_pool_size=5, label_style="soft")
    opt = types.SimpleNamespace(double_branch=True, kl_intra_weight=0.1, inher_nce_weight=0.04, explore_nce_weight=0.04,
                                collection="tiny", alpha=0.8, belta=0.8, device=torch.device(DEV), bsz=8, pin_memory=False,
                                num_workers=0, lr=1e-3, wd=0.01, lr_warmup_proportion=0.05, n_epoch=5, max_es_cnt=10,
                                hard_negative_start_epoch=0, hard_pool_size=5, distill_loss_decay="exp", exponential_k=0.95,
                                selfDistil_sigmoid_k=800, alpha_decay="sigmoid", belta_decay="sigmoid", grad_clip=-1,
                                eval_context_bsz=16, eval_query_bsz=50, eval_untrained=True,
                                ckpt_filepath=str(tmp_path / f"model_{precision}_{train_precision}.ckpt"))
    if train_precision is not None:
        opt.train_precision = train_precision
    torch.manual_seed(0)
    m = DLDKD(cfg, opt)
    ops.set_gemm_precision(precision)
    try:
        return T.train(m, ds, L(ds.videos()), L(ds.texts()), opt)
    finally:
        ops.set_gemm_precision("fp32")


def test_throughput_mode_training_learns_like_parity_mode(tmp_path):
    """Same data, seeds and schedule with every GEMM on bf16 MFMA: the loss curve tracks the parity-mode curve and
    retrieval improves as much (bf16 operand rounding must not change what is learned)."""
    ref = _fit("fp32", tmp_path)
    got = _fit("bf16", tmp_path)
    l_ref = [h[1]["loss_overall"] for h in ref[1:]]
    l_got = [h[1]["loss_overall"] for h in got[1:]]
    assert all(np.isfinite(l_got)) and l_got[-1] < l_got[0]
    for i, (a, b) in enumerate(zip(l_got, l_ref)):
        # the first epochs track closely (measured 3.8741/3.8736, 1.0748/1.0743, 0.33767/0.33762 with the fused training
        # simpool; 3.876/3.874, 1.079/1.074, 0.348/0.338 before it); later the two runs are different trajectories of the
        # same noisy optimisation (0.32/0.20, 0.21/0.13 one run; 0.25/0.20, 0.16/0.13 another): only "keeps falling" is checked
        # (round 3: the stepper pads the word / clip axes to its buckets, which re-indexes the dropout masks: 3.8572/3.8563,
        # 1.0631/1.0619, then 0.307/0.252 - the trajectories part one epoch earlier than with the round-2 masks)
        if i < 2:
            assert abs(a - b) <= 0.01 * abs(b) + 0.005, (l_got, l_ref)
        elif i == 2:
            assert abs(a - b) <= 0.3 * abs(b) + 0.02, (l_got, l_ref)
        else:
            assert a < l_got[2] and a < 3.0 * b + 0.05, (l_got, l_ref)
    s_ref, s_got = [h[2] for h in ref], [h[2] for h in got]
    assert max(s_got[1:]) > s_got[0] + 20 and max(s_got[1:]) >= max(s_ref[1:]) - 25, (s_got, s_ref)


def test_data_parallel_step_on_one_rank_rccl_group(tmp_path, rccl_comm):
    """The DDP branch of train_step (flat gradient bucket all-reduced over RCCL) with a one-rank communicator forced on:
    identical history to the plain run (mean over one rank is the identity)."""
    from dldkd_amd import train as T
    old = T.DDP_MIN_WORLD
    T.DDP_MIN_WORLD = 2
    try:
        ref = _fit("fp32", tmp_path)                      # the one-rank communicator is installed, the data-parallel branch is off
    finally:
        T.DDP_MIN_WORLD = old
    T.DDP_MIN_WORLD = 1
    try:
        got = _fit("fp32", tmp_path)
    finally:
        T.DDP_MIN_WORLD = old
    for a, b in zip(got[1:], ref[1:]):
        # not bitwise: split-K weight gradients and LayerNorm gamma/beta gradients accumulate with fp32 atomics, whose
        # order differs run to run; the difference stays at rounding level over the five epochs
        assert a[1]["loss_overall"] == pytest.approx(b[1]["loss_overall"], rel=2e-3)


def test_data_parallel_run_with_variable_caption_counts_on_one_rank(tmp_path, rccl_comm):
    """train() on a set whose videos carry 1..3 captions (every batch its own query count: the stepper pads the query axis and the
    losses read the real count from the step's staged words) with the data-parallel branch forced on over a one-rank RCCL group:
    the history of the plain run - the all-reduce between the backward graphs and the optimizer graph changes nothing else."""
    from dldkd_amd import train as T
    ds = TinySet(caps=lambda i: 1 + (i * 7) % 3)
    old = T.DDP_MIN_WORLD
    hist = []
    for world in (2, 1):
        T.DDP_MIN_WORLD = world
        try:
            hist.append(_fit("fp32", tmp_path, ds=ds))
        finally:
            T.DDP_MIN_WORLD = old
    ref, got = hist
    assert len(ref) == len(got) == 6
    for a, b in zip(got[1:3], ref[1:3]):                  # (first epochs: before run-to-run rounding has been amplified)
        assert a[1]["loss_overall"] == pytest.approx(b[1]["loss_overall"], rel=5e-3)
    assert all(np.isfinite(h[1]["loss_overall"]) for h in got[1:]) and got[-1][1]["loss_overall"] < got[1][1]["loss_overall"]


def test_train_takes_its_precision_from_opt_and_mixed_tracks_parity(tmp_path):
    """opt.train_precision = "mixed" (fp32-grade forward, bf16 backward): train() sets and restores the precision itself, and the run
    follows the parity run like the throughput run does (same data, seeds, schedule) - with loss values that ARE parity-grade."""
    from dldkd_amd import ops
    ref = _fit("fp32", tmp_path)
    got = _fit("fp32", tmp_path, train_precision="mixed")
    assert ops.precision_mode() == "fp32"                                   # restored
    l_ref = [h[1]["loss_overall"] for h in ref[1:]]
    l_got = [h[1]["loss_overall"] for h in got[1:]]
    assert all(np.isfinite(l_got)) and l_got[-1] < l_got[0]
    assert abs(l_got[0] - l_ref[0]) <= 2e-3 * abs(l_ref[0]) + 1e-3, (l_got, l_ref)     # first epoch: same parameters' worth of steps
    assert abs(l_got[1] - l_ref[1]) <= 0.01 * abs(l_ref[1]) + 0.005, (l_got, l_ref)
    s_ref, s_got = [h[2] for h in ref], [h[2] for h in got]
    assert max(s_got[1:]) > s_got[0] + 20 and max(s_got[1:]) >= max(s_ref[1:]) - 25, (s_got, s_ref)


@pytest.mark.parametrize("prec,drop", [("fp32", 0.0), ("fp32", 0.2), ("bf16", 0.2), ("mixed", 0.2)])
def test_graphed_train_step_equals_eager(prec, drop):
    """train.GraphedTrainStep (zero_grad / forward / backward / fused BertAdam replayed from ONE hipGraph, method/train.py:141-151)
    against the eager step.  Two replicas; before EVERY step the graphed replica is given the eager replica's parameters,
    moments and step count, both get the same seeds, and after the step losses and parameters must agree to rounding -
    with dropout (device Philox state: every replay draws fresh masks, the ones the eager run draws), with the reference's
    CPU randint draws for the triplet negatives (staged per step), across a switch of the baked-in hard-negative mode (a new
    graph) and a move of the epoch schedule's alpha / belta / KD weight (NO new graph: device words), and with three different
    batches flowing through one captured graph.  (Whole trajectories are not compared:
    this tiny problem amplifies the run-to-run rounding of the fp32-atomic reductions by orders of magnitude in a few
    steps - two EAGER runs diverge the same way.)"""
    import synth
    from dldkd_amd import ops
    from dldkd_amd import train as T
    from dldkd_amd.model import DLDKD
    from dldkd_amd.optimization import BertAdam
    cfg = types.SimpleNamespace(visual_input_size=256, query_input_size=128, inheritance_hidden=384, exploration_hidden=384,
                                max_ctx_l=32, max_desc_l=30, input_drop=drop, drop=drop, n_heads=4, initializer_range=0.02,
                                margin=0.1, use_hard_negative=False, hard_pool_size=20, label_style="soft")
    mopt = types.SimpleNamespace(double_branch=True, kl_intra_weight=0.1, inher_nce_weight=0.04, explore_nce_weight=0.04,
                                 collection="tvr", alpha=0.8, belta=0.8)
    topt = types.SimpleNamespace(grad_clip=-1)
    batches = [synth.make_train_batch(70 + i, nv=24, caps=2, L=20, len_lo=3, dv=256, dq=128) for i in range(3)]
    batches = [{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in b.items()} for b in batches]

    def make():
        torch.manual_seed(11)
        m = DLDKD(types.SimpleNamespace(**vars(cfg)), mopt).to(DEV).train()       # set_hard_negative() mutates the config
        return m, BertAdam([{"params": list(m.parameters()), "weight_decay": 0.01}], lr=2e-3, warmup=0.1, t_total=40)

    ops.set_gemm_precision(prec)
    try:
        me, oe = make()
        mg, og = make()
        stepper = T.GraphedTrainStep(mg, og, topt)
        tol = 1e-5 if prec == "fp32" else 1e-3
        for it in range(12):
            if it == 6:
                for m in (me, mg):
                    m.set_hard_negative(True, 5)          # per-epoch switch (train.py:62-64): a new graph key
                    m.alpha, m.weight = 0.6, 0.9
            if it == 9:
                for m in (me, mg):                        # an epoch's schedule (train.py:66-113): NO new graph - the captured loss
                    m.alpha, m.belta, m.weight = 0.45, 0.7, 0.81     # launches read these from device words (ScheduleWords)
            og.fp.flat.copy_(oe.fp.flat); og.m.copy_(oe.m); og.v.copy_(oe.v); og.step_count = oe.step_count
            torch.manual_seed(100 + it)
            # the stepper pads the clip axis (20 -> 32) and the word axis to its buckets.  Without dropout that is exact, so
            # the eager replica gets the RAW batch; with dropout the Philox masks are indexed by position in the (padded)
            # tensors, so the eager replica gets the same padded batch
            le, _ = T.train_step(me, batches[it % 3] if drop == 0.0 else stepper._bucketed(batches[it % 3]), oe, topt)
            torch.manual_seed(100 + it)
            lg, dg = stepper(batches[it % 3])
            assert float(le) == pytest.approx(float(lg), rel=tol), it
            assert dg["loss_overall"] == pytest.approx(float(lg))
            d = (oe.fp.flat - og.fp.flat).abs().max().item()
            # one Adam step moves a weight by at most ~lr; rounding-level gradient differences move it by far less
            assert d <= (2e-7 if prec == "fp32" else 2e-5) + 0.02 * og.get_lr()[0], (it, d)
            assert og.step_count == oe.step_count
    finally:
        ops.set_gemm_precision("fp32")
    assert stepper.replays == 10 and stepper.captures == 2 and stepper.eager_steps == 2     # each key: 1 eager sight, then captured


@pytest.mark.parametrize("words", [True, False])
def test_one_captured_step_serves_every_epoch_of_the_schedule(words, monkeypatch):
    """train_epoch moves alpha / belta / the KD weight every epoch (method/train.py:66-113).  With the schedule's scalars as device
    words (GraphedTrainStep.SCHEDULE_WORDS, functional.ScheduleWords) the step captured in epoch 0 is replayed in every epoch; with
    the scalars baked in (the fallback) every epoch costs an eager step + a capture - and a 100-epoch run would leave the graphs
    after max_captures epochs."""
    from dldkd_amd.model import DLDKD
    from dldkd_amd import train as T
    ds = TinySet()
    cfg = types.SimpleNamespace(visual_input_size=256, query_input_size=128, inheritance_hidden=384, exploration_hidden=384,
                                max_ctx_l=128, max_desc_l=30, input_drop=0.1, drop=0.1, n_heads=4, initializer_range=0.02,
                                margin=0.1, use_hard_negative=False, hard_pool_size=5, label_style="soft")
    opt = types.SimpleNamespace(double_branch=True, kl_intra_weight=0.1, inher_nce_weight=0.04, explore_nce_weight=0.04,
                                collection="tiny", alpha=0.8, belta=0.8, device=torch.device(DEV), bsz=8, pin_memory=False,
                                num_workers=0, lr=1e-3, wd=0.01, lr_warmup_proportion=0.05, n_epoch=4, max_es_cnt=10,
                                hard_negative_start_epoch=0, hard_pool_size=5, distill_loss_decay="exp", exponential_k=0.9,
                                selfDistil_sigmoid_k=8, alpha_decay="sigmoid", belta_decay="sigmoid", grad_clip=-1,
                                prefetch_batches=False)          # (one capture per signature: the count below is about the schedule)
    monkeypatch.setattr(T.GraphedTrainStep, "SCHEDULE_WORDS", words)
    torch.manual_seed(0)
    m = DLDKD(cfg, opt).to(DEV)
    loader = T.make_train_loader(ds, opt, 0, 1)
    optim = T.make_optimizer(m, opt, len(loader))
    stepper = T.GraphedTrainStep(m, optim, opt, defer_loss_float=True)
    seen, losses = [], []
    for ep in range(4):
        losses.append(T.train_epoch(m, loader, optim, opt, ep, stepper=stepper)["loss_overall"])
        seen.append((m.alpha, m.belta, m.weight))
    assert len(set(seen)) == 4 and all(np.isfinite(losses))          # the schedule moved every epoch
    n = 4 * len(loader)
    if words:
        assert (stepper.captures, stepper.eager_steps, stepper.replays) == (1, 1, n - 1)
    else:
        assert (stepper.captures, stepper.eager_steps, stepper.replays) == (4, 4, n - 4)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_double_buffered_inputs_give_the_same_steps(prec):
    """GraphedTrainStep(batch, next_batch=...): the next step's inputs are copied into a SECOND set of static buffers (a second
    capture of the same signature) on the staging stream while this step runs.  Against a stepper that stages every batch at the
    head of its own step: same losses and parameters step by step (the plain stepper's state is copied over before every step, same
    seeds: dropout masks and triplet draws are the same), with a batch of another signature in the stream (that step stages its
    inputs itself) and a caller that breaks its promise once (the prefetched inputs are ignored, not used for the wrong batch)."""
    import synth
    from dldkd_amd import ops
    from dldkd_amd import train as T
    from dldkd_amd.model import DLDKD
    from dldkd_amd.optimization import BertAdam
    cfg = types.SimpleNamespace(visual_input_size=256, query_input_size=128, inheritance_hidden=384, exploration_hidden=384,
                                max_ctx_l=32, max_desc_l=30, input_drop=0.2, drop=0.2, n_heads=4, initializer_range=0.02,
                                margin=0.1, use_hard_negative=True, hard_pool_size=5, label_style="soft")
    mopt = types.SimpleNamespace(double_branch=True, kl_intra_weight=0.1, inher_nce_weight=0.04, explore_nce_weight=0.04,
                                 collection="tvr", alpha=0.8, belta=0.8)
    topt = types.SimpleNamespace(grad_clip=-1, device=torch.device(DEV))
    batches = [synth.make_train_batch(170 + i, nv=24, caps=2, L=20, len_lo=3, dv=256, dq=128) for i in range(4)]
    batches.append(synth.make_train_batch(180, nv=16, caps=2, L=20, len_lo=3, dv=256, dq=128))      # another signature
    batches = [{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in b.items()} for b in batches]
    order = [0, 1, 2, 3, 0, 1, 2, 4, 3, 0, 1, 2, 3, 0, 1, 2]
    lie_at = 10                                            # promised batches[order[11]], delivers batches[3]

    def make():
        torch.manual_seed(11)
        m = DLDKD(types.SimpleNamespace(**vars(cfg)), mopt).to(DEV).train()
        return m, BertAdam([{"params": list(m.parameters()), "weight_decay": 0.01}], lr=2e-3, warmup=0.1, t_total=40)

    ops.set_gemm_precision(prec)
    try:
        mp, op_ = make()
        md, od = make()
        plain, dbl = T.GraphedTrainStep(mp, op_, topt), T.GraphedTrainStep(md, od, topt)
        plain.QUERY_BUCKET = dbl.QUERY_BUCKET = 0          # (the two signatures differ in their query counts: no query padding in this test)
        tol = 1e-5 if prec == "fp32" else 1e-3
        seq = list(order)
        for it in range(len(seq)):
            if it == lie_at + 1:
                seq[it] = 3
            b = batches[seq[it]]
            nxt = batches[order[it + 1]] if it + 1 < len(order) else None
            od.fp.flat.copy_(op_.fp.flat); od.m.copy_(op_.m); od.v.copy_(op_.v); od.step_count = op_.step_count
            torch.manual_seed(300 + it)
            lp, _ = plain(b)
            torch.manual_seed(300 + it)
            ld, _ = dbl(b, next_batch=nxt)
            assert float(lp) == pytest.approx(float(ld), rel=tol), it
            d = (op_.fp.flat - od.fp.flat).abs().max().item()
            assert d <= (2e-7 if prec == "fp32" else 2e-5) + 0.02 * od.get_lr()[0], (it, d)
    finally:
        ops.set_gemm_precision("fp32")
    # two captures of the main signature (its two buffer sets); the other signature and the broken promise staged their own inputs
    assert dbl.double_buffer and dbl.captures == 2 and plain.captures == 1
    assert dbl.prefetched >= len(order) - 9, dbl.prefetched
    assert dbl.replays + dbl.eager_steps == len(order) + 0


def test_train_epoch_prefetches_the_next_batch_and_follows_the_unprefetched_run():
    """train_epoch drives a graphed stepper through GraphedTrainStep.iterate: batch i + 1 is fetched on the staging stream (the
    device-resident set's gather kernels / a host loader's uploads) and copied into the other input buffer set while step i runs.
    Same data, same seeds as a run with opt.prefetch_batches = False: the epoch means agree (first epochs: before run-to-run
    rounding has been amplified), nearly every step found its inputs in place."""
    from dldkd_amd.model import DLDKD
    from dldkd_amd import train as T
    ds = TinySet()
    cfg = types.SimpleNamespace(visual_input_size=256, query_input_size=128, inheritance_hidden=384, exploration_hidden=384,
                                max_ctx_l=128, max_desc_l=30, input_drop=0.1, drop=0.1, n_heads=4, initializer_range=0.02,
                                margin=0.1, use_hard_negative=False, hard_pool_size=5, label_style="soft")
    res = {}
    for resident in (False, True):
        for ahead in (False, True):
            opt = types.SimpleNamespace(double_branch=True, kl_intra_weight=0.1, inher_nce_weight=0.04, explore_nce_weight=0.04,
                                        collection="tiny", alpha=0.8, belta=0.8, device=torch.device(DEV), bsz=8, pin_memory=False,
                                        num_workers=0, lr=1e-3, wd=0.01, lr_warmup_proportion=0.05, n_epoch=4, max_es_cnt=10,
                                        hard_negative_start_epoch=0, hard_pool_size=5, distill_loss_decay="exp", exponential_k=0.9,
                                        selfDistil_sigmoid_k=8, alpha_decay="sigmoid", belta_decay="sigmoid", grad_clip=-1,
                                        prefetch_batches=ahead, device_resident_train=resident)
            torch.manual_seed(0)
            m = DLDKD(cfg, opt).to(DEV)
            loader = T.make_train_loader(ds, opt, 0, 1)
            optim = T.make_optimizer(m, opt, len(loader))
            stepper = T.GraphedTrainStep(m, optim, opt, defer_loss_float=True)
            torch.manual_seed(5)
            losses = [T.train_epoch(m, loader, optim, opt, ep, stepper=stepper)["loss_overall"] for ep in range(4)]
            res[(resident, ahead)] = (losses, stepper)
    for resident in (False, True):
        (l0, s0), (l1, s1) = res[(resident, False)], res[(resident, True)]
        assert s0.prefetched == 0 and not s0.double_buffer
        # 12 steps: 2 first sights + 2 captures stage their own inputs; a step after an epoch's last batch has nothing ahead of it
        assert s1.double_buffer and s1.captures == 2 and s1.prefetched >= 5, (s1.captures, s1.prefetched)
        assert abs(l0[0] - l1[0]) <= 2e-3 * abs(l0[0]) + 1e-3 and abs(l0[1] - l1[1]) <= 0.01 * abs(l0[1]) + 0.005, (l0, l1)
        assert all(np.isfinite(l1))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_variable_caption_counts_share_a_captured_step(prec):
    """Charades / ActivityNet batches hold a different number of captions each (data_provider.py:34-72), i.e. a different query
    count per batch: every batch its own graph signature, and GraphedTrainStep would never replay.  The stepper pads the QUERY axis
    to a multiple of 32 (one-word zero queries behind the real ones); towers and pooled scores run over all rows, the fused losses
    over the real ones (dldkd_branch_losses_f32 nq_valid, read from the step's device words).  (a) the model on a padded batch =
    the model on the raw batch: losses and gradients (no dropout; both eager); (b) ten batches of several different query counts in
    one bucket: ONE capture, eight replays (padding starts with the second distinct count), each step equal to the eager step on the
    same batch (state copied over before every step, same seeds), with dropout on."""
    import synth
    from dldkd_amd import ops
    from dldkd_amd import train as T
    from dldkd_amd.model import DLDKD
    from dldkd_amd.optimization import BertAdam
    mopt = types.SimpleNamespace(double_branch=True, kl_intra_weight=0.1, inher_nce_weight=0.04, explore_nce_weight=0.04,
                                 collection="charades", alpha=0.8, belta=0.8)
    topt = types.SimpleNamespace(grad_clip=-1)

    def cfg(drop):
        return types.SimpleNamespace(visual_input_size=256, query_input_size=128, inheritance_hidden=384, exploration_hidden=384,
                                     max_ctx_l=32, max_desc_l=30, input_drop=drop, drop=drop, n_heads=4, initializer_range=0.02,
                                     margin=0.1, use_hard_negative=True, hard_pool_size=5, label_style="soft")

    def batch(seed, counts):
        b = synth.make_train_batch(seed, nv=len(counts), caps=sorted(counts, reverse=True), L=32, len_lo=3, dv=256, dq=128, lq_hi=24)
        return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in b.items()}

    rs = np.random.RandomState(3)
    ops.set_gemm_precision(prec)
    try:
        # (a)
        torch.manual_seed(11)
        m = DLDKD(cfg(0.0), mopt).to(DEV).train()
        raw = batch(400, [3] * 6 + [2] * 10 + [1] * 8)              # 46 queries -> 64 rows
        stepper = T.GraphedTrainStep(m, BertAdam([{"params": list(m.parameters()), "weight_decay": 0.01}], lr=1e-3, warmup=0.1, t_total=40), topt)
        assert stepper._bucketed(raw) is raw and not stepper.vary_queries      # one query count seen so far: nothing to pad for
        stepper.vary_queries = True
        pad = stepper._bucketed(raw)
        assert pad["student_text"].shape[0] == 64 and len(pad["text_labels"]) == 46 and pad["teacher_text"].shape[0] == 64
        assert float(pad["student_text_mask"][46:].sum()) == 18.0 and float(pad["student_text"][46:].abs().max()) == 0.0
        res = []
        for b in (raw, pad):
            m.zero_grad(set_to_none=True)
            torch.manual_seed(5)
            loss, parts = m(b)
            loss.backward()
            res.append((float(loss), {k: float(v) for k, v in parts.items()}, [p.grad.clone() for p in m.parameters()]))
        tol = 1e-5 if prec == "fp32" else 2e-3
        assert res[0][0] == pytest.approx(res[1][0], rel=tol)
        for k in res[0][1]:
            assert res[0][1][k] == pytest.approx(res[1][1][k], rel=tol, abs=1e-7), k
        for (n, _), a, b in zip(m.named_parameters(), res[0][2], res[1][2]):
            assert (a - b).norm().item() <= (1e-4 if prec == "fp32" else 2e-2) * max(a.norm().item(), 1e-6) + 1e-7, n
        # (b)
        def make():
            torch.manual_seed(12)
            mm = DLDKD(cfg(0.2), mopt).to(DEV).train()
            return mm, BertAdam([{"params": list(mm.parameters()), "weight_decay": 0.01}], lr=2e-3, warmup=0.1, t_total=40)
        me, oe = make()
        mg, og = make()
        g = T.GraphedTrainStep(mg, og, topt)
        counts = [[int(c) for c in rs.randint(1, 4, size=24)] for _ in range(10)]
        nqs = [sum(c) for c in counts]
        assert len(set(nqs)) >= 5 and len({-(-n // 32) * 32 for n in nqs}) == 1, nqs
        for it, c in enumerate(counts):
            b = batch(500 + it, c)
            og.fp.flat.copy_(oe.fp.flat); og.m.copy_(oe.m); og.v.copy_(oe.v); og.step_count = oe.step_count
            torch.manual_seed(700 + it)
            le, _ = T.train_step(me, g._bucketed(b), oe, topt)      # (dropout masks are indexed by position in the padded tensors)
            torch.manual_seed(700 + it)
            lg, _ = g(b)
            assert float(le) == pytest.approx(float(lg), rel=1e-5 if prec == "fp32" else 1e-3), it
            d = (oe.fp.flat - og.fp.flat).abs().mean().item()
            assert d <= 1e-7 + 0.02 * og.get_lr()[0], (it, d)
        # (batches run unpadded until a second query count appears - here the first two happen to hold the same count, so the unpadded
        # signature is captured too - then the padded signature: one eager sight, one capture, replays)
        assert g.vary_queries and g.captures <= 2 and g.eager_steps <= 2 and g.replays >= 8, (g.captures, g.eager_steps, g.replays)
        assert sorted(e.nq for e in g.graphs.values())[-1] == 64
    finally:
        ops.set_gemm_precision("fp32")


def test_graphed_step_serves_variable_length_batches_from_a_few_graphs():
    """real loaders pad every batch to ITS longest caption / video, so raw shapes change from batch to
    batch.  The stepper buckets the word / clip axes (exact: no dropout here, every step is compared with the eager step on the
    RAW batch), stages the labels per step (batches with the same shapes but another caption -> video map replay the same
    graph), never re-captures an evicted key and stops capturing after max_captures: replays must far exceed captures."""
    import synth
    from dldkd_amd import train as T
    from dldkd_amd.model import DLDKD
    from dldkd_amd.optimization import BertAdam
    cfg = types.SimpleNamespace(visual_input_size=256, query_input_size=128, inheritance_hidden=384, exploration_hidden=384,
                                max_ctx_l=128, max_desc_l=30, input_drop=0.0, drop=0.0, n_heads=4, initializer_range=0.02,
                                margin=0.1, use_hard_negative=True, hard_pool_size=5, label_style="soft")
    mopt = types.SimpleNamespace(double_branch=True, kl_intra_weight=0.1, inher_nce_weight=0.04, explore_nce_weight=0.04,
                                 collection="tvr", alpha=0.8, belta=0.8)
    topt = types.SimpleNamespace(grad_clip=-1)
    rs = np.random.RandomState(0)
    batches = []
    for i in range(28):
        L = int(rs.choice([40, 70, 100, 128, 33, 64, 90, 120]))
        b = synth.make_train_batch(300 + i, nv=16, caps=2, L=L, len_lo=3, dv=256, dq=128, lq_lo=4, lq_hi=int(rs.randint(10, 31)))
        if i % 2:                                                    # same shapes family, another caption -> video map
            perm = torch.from_numpy(rs.permutation(len(b["text_labels"])))
            for k in ("student_text", "student_text_mask", "teacher_text"):
                b[k] = b[k][perm]
            b["text_labels"] = [b["text_labels"][j] for j in perm.tolist()]
        batches.append({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in b.items()})
    assert len({(tuple(b["student_text"].shape), tuple(b["student_videos"].shape)) for b in batches}) >= 12   # raw signatures

    def make():
        torch.manual_seed(11)
        m = DLDKD(types.SimpleNamespace(**vars(cfg)), mopt).to(DEV).train()
        return m, BertAdam([{"params": list(m.parameters()), "weight_decay": 0.01}], lr=1e-3, warmup=0.1, t_total=200)
    me, oe = make()
    mg, og = make()
    stepper = T.GraphedTrainStep(mg, og, topt, max_graphs=3, max_captures=5)
    for rep in range(3):
        for it, b in enumerate(batches):
            og.fp.flat.copy_(oe.fp.flat); og.m.copy_(oe.m); og.v.copy_(oe.v); og.step_count = oe.step_count
            torch.manual_seed(500 + it)
            le, _ = T.train_step(me, b, oe, topt)
            torch.manual_seed(500 + it)
            lg, _ = stepper(b)
            assert float(le) == pytest.approx(float(lg), rel=2e-5), (rep, it)
            assert (oe.fp.flat - og.fp.flat).abs().max().item() <= 2e-7 + 0.02 * og.get_lr()[0]
    n = 3 * len(batches)
    assert stepper.captures <= 5 and stepper.replays + stepper.eager_steps == n
    assert stepper.replays >= 6 * stepper.captures, (stepper.replays, stepper.captures, stepper.eager_steps)
    assert len(stepper.graphs) <= 3 and not (set(stepper.graphs) & stepper.evicted)


@pytest.mark.parametrize("drop", [0.0, 0.2])
def test_data_parallel_stepper_runs_the_step_as_a_chain_of_graph_segments(drop, rccl_comm):
    """Data parallel (one-rank RCCL group forced on, gradient buckets per tower): the stepper replays the step as a chain of
    graphs - one per tower of the backward pass, each tower's all-reduce issued from the comm stream behind its segment - plus
    the optimizer graph.  Against the plain single-graph stepper on the same seeds: same loss and parameters after every
    step (a mean over one rank is the identity), with dropout too; eager data-parallel steps (phased backward) agree as well."""
    import synth
    from dldkd_amd import train as T
    from dldkd_amd.model import DLDKD
    from dldkd_amd.optimization import BertAdam
    cfg = types.SimpleNamespace(visual_input_size=256, query_input_size=128, inheritance_hidden=384, exploration_hidden=384,
                                max_ctx_l=32, max_desc_l=30, input_drop=drop, drop=drop, n_heads=4, initializer_range=0.02,
                                margin=0.1, use_hard_negative=True, hard_pool_size=5, label_style="soft")
    mopt = types.SimpleNamespace(double_branch=True, kl_intra_weight=0.1, inher_nce_weight=0.04, explore_nce_weight=0.04,
                                 collection="tvr", alpha=0.8, belta=0.8)
    topt = types.SimpleNamespace(grad_clip=-1)
    batches = [synth.make_train_batch(170 + i, nv=24, caps=2, L=32, len_lo=3, dv=256, dq=128, lq_lo=6, lq_hi=30) for i in range(3)]
    batches = [{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in b.items()} for b in batches]

    def make(buckets):
        torch.manual_seed(11)
        m = DLDKD(types.SimpleNamespace(**vars(cfg)), mopt).to(DEV).train()
        return m, BertAdam([{"params": list(m.parameters()), "weight_decay": 0.01}], lr=2e-3, warmup=0.1, t_total=40,
                           grad_buckets=m.grad_buckets() if buckets else None)

    def params(m):
        return torch.cat([p.detach().reshape(-1) for p in m.parameters()])

    def give(dst_m, dst_o, src_m, src_o):                  # parameters and moments by NAME: the two flat layouts differ
        for (pd, ps) in zip(dst_m.parameters(), src_m.parameters()):
            pd.data.copy_(ps.data)
        for name in ("m", "v"):
            for i in range(len(dst_o.fp.params)):
                sd, ns = dst_o.fp._starts[i], dst_o.fp._numels[i]
                ss = src_o.fp._starts[i]
                getattr(dst_o, name)[sd:sd + ns].copy_(getattr(src_o, name)[ss:ss + ns])
        dst_o.step_count = src_o.step_count

    mp_, op_ = make(False)
    old = T.DDP_MIN_WORLD
    T.DDP_MIN_WORLD = 2
    plain = T.GraphedTrainStep(mp_, op_, topt)
    T.DDP_MIN_WORLD = 1
    try:
        md, od = make(True)
        assert len(od.fp.bucket_ranges) == 4 and od.fp.bucket_ranges[-1][1] == od.fp.total
        ddp = T.GraphedTrainStep(md, od, topt)
        me, oe = make(True)
        for it in range(8):
            give(md, od, mp_, op_)
            give(me, oe, mp_, op_)
            T.DDP_MIN_WORLD = 2
            torch.manual_seed(300 + it)
            lp, _ = plain(batches[it % 3])
            T.DDP_MIN_WORLD = 1
            torch.manual_seed(300 + it)
            ld, dd = ddp(batches[it % 3])
            torch.manual_seed(300 + it)
            # (the stepper pads the 48 queries to its bucket of 64; the dropout masks are indexed by position in the padded tensors)
            le, _ = T.train_step(me, plain._bucketed(batches[it % 3]), oe, topt)
            assert float(lp) == pytest.approx(float(ld), rel=1e-5), it
            assert float(lp) == pytest.approx(float(le), rel=1e-5), it
            tol = 2e-7 + 0.02 * od.get_lr()[0]
            assert (params(mp_) - params(md)).abs().max().item() <= tol, it
            assert (params(mp_) - params(me)).abs().max().item() <= tol, it
            assert od.step_count == op_.step_count
        assert ddp.replays == 7 and ddp.captures == 1 and ddp.eager_steps == 1
        e = next(iter(ddp.graphs.values()))
        assert len(e.segments) == 4 and e.opt_graph is not None
    finally:
        T.DDP_MIN_WORLD = old


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_tower_streams_at_c3_size_match_single_stream(prec):
    """The stepper forks the four towers onto four streams (model._encode_towers) - at the TVR batch size (128 videos x 128
    clips x 3072, 640 queries), where the towers' kernels really overlap.  40 steps, dropout on, three batches; before every step
    the stepper's replica gets the single-stream eager replica's state, after it losses and parameters must agree to the
    rounding of the fp32-atomic reductions.  A cross-stream race (a buffer recycled while another stream still reads it, a
    missing join) shows up as a parameter off by far more than one Adam step can move it."""
    import synth
    from dldkd_amd import ops
    from dldkd_amd import train as T
    from dldkd_amd.model import DLDKD
    from dldkd_amd.optimization import BertAdam
    cfg = types.SimpleNamespace(visual_input_size=3072, query_input_size=768, inheritance_hidden=384, exploration_hidden=384,
                                max_ctx_l=128, max_desc_l=30, input_drop=0.2, drop=0.2, n_heads=4, initializer_range=0.02,
                                margin=0.1, use_hard_negative=True, hard_pool_size=20, label_style="soft")
    mopt = types.SimpleNamespace(double_branch=True, kl_intra_weight=0.1, inher_nce_weight=0.04, explore_nce_weight=0.04,
                                 collection="tvr", alpha=0.8, belta=0.8)
    topt = types.SimpleNamespace(grad_clip=-1)
    batches = [synth.make_train_batch(900 + i, nv=128, caps=5, L=128, len_lo=24, dv=3072, dq=768, lq_lo=6, lq_hi=30) for i in range(3)]
    batches = [{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in b.items()} for b in batches]

    def make():
        torch.manual_seed(21)
        m = DLDKD(types.SimpleNamespace(**vars(cfg)), mopt).to(DEV).train()
        return m, BertAdam([{"params": list(m.parameters()), "weight_decay": 0.01}], lr=3e-4, warmup=0.1, t_total=400)

    ops.set_gemm_precision(prec)
    try:
        me, oe = make()
        mg, og = make()
        stepper = T.GraphedTrainStep(mg, og, topt)
        assert mg.tower_streams and not me.tower_streams
        worst = 0.0
        for it in range(40):
            og.fp.flat.copy_(oe.fp.flat); og.m.copy_(oe.m); og.v.copy_(oe.v); og.step_count = oe.step_count
            torch.manual_seed(700 + it)
            le, _ = T.train_step(me, batches[it % 3], oe, topt)
            torch.manual_seed(700 + it)
            lg, _ = stepper(batches[it % 3])
            assert float(le.detach()) == pytest.approx(float(lg), rel=2e-5 if prec == "fp32" else 1e-3), it
            d = (oe.fp.flat - og.fp.flat).abs().max().item()
            worst = max(worst, d)
            assert d <= (2e-7 if prec == "fp32" else 2e-5) + 0.05 * og.get_lr()[0], (it, d)
        assert stepper.replays >= 38
    finally:
        ops.set_gemm_precision("fp32")


def test_device_resident_train_set_yields_the_collated_batches():
    """data.DeviceTrainSet / DeviceTrainLoader (the training items read once into ragged device tables, batches gathered by
    dldkd_gather_pad_rows_f32) against DataLoader + collate_train + .to(device): the same batches - tensors bit for bit, labels,
    order - epoch after epoch under the same seed (the index-only DataLoader makes the same draws from the global generator),
    with variable caption counts (collate_train's stable most-captions-first order) and a ragged last batch."""
    from torch.utils.data import DataLoader
    from dldkd_amd.data import DeviceTrainLoader, DeviceTrainSet, collate_train
    ds = TinySet(n=37)
    g = torch.Generator().manual_seed(3)
    for i in range(0, 37, 3):                     # a third caption on some videos, one caption on others
        it = list(ds.items[i])
        if i % 2:
            it[1], it[3], it[5] = it[1][:1], it[3][:1], it[5][:1]
        else:
            it[1] = it[1] + [torch.nn.functional.normalize(torch.randn(7, it[1][0].shape[1], generator=g), dim=-1)]
            it[3] = it[3] + [it[3][0] * 0.5]
            it[5] = it[5] + [it[5][0] + "x"]
        ds.items[i] = tuple(it)
    devset = DeviceTrainSet(ds, DEV)
    assert len(devset) == 37 and devset.n_caps == sum(len(it[1]) for it in ds.items)
    by_workers = DeviceTrainSet(ds, DEV, num_workers=2)        # (the reading pass with loader workers: tables concatenated in the worker)
    assert by_workers.caps_of == devset.caps_of and all(torch.equal(by_workers.src[k], devset.src[k]) for k in devset.TABLES)
    assert all(np.array_equal(by_workers.lens_host[k], devset.lens_host[k]) for k in devset.TABLES)
    del by_workers
    for epoch in range(2):
        torch.manual_seed(100 + epoch)
        ref = list(DataLoader(ds, batch_size=8, shuffle=True, num_workers=0, collate_fn=collate_train))
        after_ref = torch.rand(1)
        torch.manual_seed(100 + epoch)
        got = list(DeviceTrainLoader(devset, 8, shuffle=True))
        assert torch.equal(after_ref, torch.rand(1))                      # the global generator is where the DataLoader leaves it
        assert len(got) == len(ref) == 5
        for a, b in zip(got, ref):
            assert a["text_labels"] == b["text_labels"]
            for k in ("student_videos", "teacher_videos", "student_videos_mask", "student_text", "student_text_mask", "teacher_text"):
                assert a[k].is_cuda and torch.equal(a[k].cpu(), b[k]), k
    # plan + gather into a caller's buffers with padding (what train.GraphedTrainStep.iterate does with a captured step's input
    # buffers): the same rows, zero rows / zero mask behind them, written in place; the plans follow the loader's order and draws
    import torch.nn.functional as TF
    torch.manual_seed(100)
    ref = list(DeviceTrainLoader(devset, 8, shuffle=True))
    torch.manual_seed(100)
    plans = list(DeviceTrainLoader(devset, 8, shuffle=True).plans())
    assert len(plans) == len(ref)
    for pl, b in zip(plans, ref):
        lv, lq = pl.lmax["student_videos"] + 5, pl.lmax["student_text"] + 3
        nv, nq = len(pl.vids), len(pl.caps)
        out = {"student_videos": torch.full((nv, lv, 256), 7.0, device=DEV), "student_videos_mask": torch.full((nv, lv), 7.0, device=DEV),
               "teacher_videos": torch.full((nv, lv, 512), 7.0, device=DEV), "student_text": torch.full((nq, lq, 128), 7.0, device=DEV),
               "student_text_mask": torch.full((nq, lq), 7.0, device=DEV), "teacher_text": torch.full((nq, 1, 512), 7.0, device=DEV)}
        got = devset.gather(pl, out=out, pad={"student_videos": lv, "teacher_videos": lv, "student_text": lq})
        assert got["text_labels"] == b["text_labels"] and all(got[k] is out[k] for k in out)
        assert torch.equal(got["student_videos"], TF.pad(b["student_videos"], (0, 0, 0, lv - b["student_videos"].shape[1])))
        assert torch.equal(got["teacher_videos"], TF.pad(b["teacher_videos"], (0, 0, 0, lv - b["teacher_videos"].shape[1])))
        assert torch.equal(got["student_videos_mask"], TF.pad(b["student_videos_mask"], (0, lv - b["student_videos_mask"].shape[1])))
        assert torch.equal(got["student_text"], TF.pad(b["student_text"], (0, 0, 0, lq - b["student_text"].shape[1])))
        assert torch.equal(got["student_text_mask"], TF.pad(b["student_text_mask"], (0, lq - b["student_text_mask"].shape[1])))
        assert torch.equal(got["teacher_text"], b["teacher_text"])
    with pytest.raises(ValueError, match="destination"):
        devset.gather(plans[0], out={"student_videos": torch.empty(3, 3, 256, device=DEV)})


def test_training_set_goes_device_resident_by_itself_when_its_items_repeat():
    """make_train_loader, opt.device_resident_train unset ("auto"): a dataset that hands out the same item on every read (the
    reference's Dataset4DLDKD) is kept on the device; one whose items change between reads (augmentation) or that does not fit the
    cap stays with the host DataLoader; the probe leaves the global generators where they were; False / True are obeyed."""
    from torch.utils.data import DataLoader
    from dldkd_amd import train as T
    from dldkd_amd.data import DeviceTrainLoader
    ds = TinySet(n=16)

    class Noisy(TinySet):
        def __getitem__(self, i):
            it = list(self.items[i])
            it[0] = it[0] + 0.01 * torch.randn_like(it[0])
            return tuple(it)

    def opt(**kw):
        return types.SimpleNamespace(device=torch.device(DEV), bsz=8, pin_memory=False, num_workers=0, **kw)
    torch.manual_seed(3)
    before = torch.get_rng_state()
    assert isinstance(T.make_train_loader(ds, opt(), 0, 1), DeviceTrainLoader)
    assert isinstance(T.make_train_loader(Noisy(n=16), opt(), 0, 1), DataLoader)
    assert torch.equal(before, torch.get_rng_state())
    assert isinstance(T.make_train_loader(ds, opt(device_resident_train=False), 0, 1), DataLoader)
    assert isinstance(T.make_train_loader(ds, opt(train_feature_cache_gb=1e-6), 0, 1), DataLoader)
    with pytest.raises(MemoryError):
        T.make_train_loader(ds, opt(device_resident_train=True, train_feature_cache_gb=1e-6), 0, 1)
    assert isinstance(T.make_train_loader(ds, types.SimpleNamespace(device="cpu", bsz=8, pin_memory=False, num_workers=0), 0, 1), DataLoader)


def test_train_with_the_device_resident_set_follows_the_host_loader_run(tmp_path):
    """train() with opt.device_resident_train: the same history (losses, SumR) as with the DataLoader + collate + H2D path."""
    from dldkd_amd.model import DLDKD
    from dldkd_amd import train as T
    hist = []
    for resident in (False, True):
        ds = TinySet()
        cfg = types.SimpleNamespace(visual_input_size=256, query_input_size=128, inheritance_hidden=384, exploration_hidden=384,
                                    max_ctx_l=128, max_desc_l=30, input_drop=0.1, drop=0.1, n_heads=4, initializer_range=0.02,
                                    margin=0.1, use_hard_negative=False, hard_pool_size=5, label_style="soft")
        opt = types.SimpleNamespace(double_branch=True, kl_intra_weight=0.1, inher_nce_weight=0.04, explore_nce_weight=0.04,
                                    collection="tiny", alpha=0.8, belta=0.8, device=torch.device(DEV), bsz=8, pin_memory=False,
                                    num_workers=0, lr=1e-3, wd=0.01, lr_warmup_proportion=0.05, n_epoch=3, max_es_cnt=10,
                                    hard_negative_start_epoch=0, hard_pool_size=5, distill_loss_decay="exp", exponential_k=0.95,
                                    selfDistil_sigmoid_k=800, alpha_decay="sigmoid", belta_decay="sigmoid", grad_clip=-1,
                                    eval_context_bsz=16, eval_query_bsz=50, eval_untrained=False, ckpt_filepath=None,
                                    device_resident_train=resident)
        torch.manual_seed(0)
        m = DLDKD(cfg, opt)
        hist.append(T.train(m, ds, L(ds.videos()), L(ds.texts()), opt))
    for a, b in zip(*hist):
        assert a[1]["loss_overall"] == pytest.approx(b[1]["loss_overall"], rel=2e-3)      # fp32-atomic reductions vary run to run
        assert abs(a[2] - b[2]) <= 12.0


def test_parallel_tower_graphs_are_used_and_match_the_single_graph():
    """One GPU: GraphedTrainStep captures the step as 3 + 2 T graphs - every tower's forward and backward pass in its own graph,
    on its own stream and memory pool - and replays the tower graphs side by side on streams that were MEASURED to have their
    own hardware queues (staging.concurrent_streams).  Against the single graph with fork / join edges (opt.parallel_tower_graphs
    = False): same losses and parameters step by step, with dropout, across two graph keys; the captured entry really is the
    multi-graph form and the four streams overlap pairwise."""
    import synth
    from dldkd_amd import ops, staging
    from dldkd_amd import train as T
    from dldkd_amd.model import DLDKD
    from dldkd_amd.optimization import BertAdam
    cfg = types.SimpleNamespace(visual_input_size=256, query_input_size=128, inheritance_hidden=384, exploration_hidden=384,
                                max_ctx_l=64, max_desc_l=30, input_drop=0.2, drop=0.2, n_heads=4, initializer_range=0.02,
                                margin=0.1, use_hard_negative=False, hard_pool_size=20, label_style="soft")
    mopt = types.SimpleNamespace(double_branch=True, kl_intra_weight=0.1, inher_nce_weight=0.04, explore_nce_weight=0.04,
                                 collection="tvr", alpha=0.8, belta=0.8)
    batches = [synth.make_train_batch(80 + i, nv=24, caps=2, L=20 + 20 * (i % 2), len_lo=3, dv=256, dq=128) for i in range(2)]
    batches = [{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in b.items()} for b in batches]

    def make(par):
        torch.manual_seed(13)
        m = DLDKD(types.SimpleNamespace(**vars(cfg), ), mopt).to(DEV).train()
        o = BertAdam([{"params": list(m.parameters()), "weight_decay": 0.01}], lr=2e-3, warmup=0.1, t_total=40)
        return m, o, T.GraphedTrainStep(m, o, types.SimpleNamespace(grad_clip=-1, parallel_tower_graphs=par))

    ops.set_gemm_precision("bf16")
    try:
        ma, oa, sa = make(True)
        mb, ob, sb = make(False)
        for it in range(10):
            ob.fp.flat.copy_(oa.fp.flat); ob.m.copy_(oa.m); ob.v.copy_(oa.v); ob.step_count = oa.step_count
            torch.manual_seed(300 + it)
            la, _ = sa(batches[it % 2])
            torch.manual_seed(300 + it)
            lb, _ = sb(batches[it % 2])
            assert float(la) == pytest.approx(float(lb), rel=1e-3), it
            assert (oa.fp.flat - ob.fp.flat).abs().max().item() <= 2e-5 + 0.05 * oa.get_lr()[0], it
        assert sa.replays >= 6 and sb.replays >= 6
        assert all(getattr(e, "par", None) for e in sa.graphs.values()) and len(sa.graphs) == 2
        assert not any(getattr(e, "par", None) for e in sb.graphs.values())
        e = next(iter(sa.graphs.values()))
        assert len(e.par["fwd"]) == len(e.par["bwd"]) == 4 and len({id(s) for s in e.par["streams"]}) == 4
        # the four streams run a one-workgroup spin kernel side by side (their own hardware queues) - as many of them as the device
        # has queues (GPU_MAX_HW_QUEUES): the stepper's streams are measured, those with a queue of their own come first
        side_by_side = e.par["streams"][:min(4, staging.hardware_queues())]
        import time
        def spin(streams):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in streams:
                with torch.cuda.stream(s):
                    torch.cuda._sleep(2_000_000)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        spin(e.par["streams"][:1])
        one = min(spin(e.par["streams"][:1]) for _ in range(3))
        assert min(spin(side_by_side) for _ in range(3)) < 1.6 * one
        assert len(staging.concurrent_streams(torch.device(DEV), 3)) == 3
    finally:
        ops.set_gemm_precision("fp32")


@pytest.mark.parametrize("prec", ["bf16", "mixed"])
def test_single_graph_stepper_at_c3_size_and_the_self_check(prec, monkeypatch):
    """The TVR-size step through the single-graph form (opt.parallel_tower_graphs = False: the fallback of the tower graphs, fork /
    join edges inside ONE capture) in the modes that run the one-pass input LayerNorm: the capture passes its self-check (round 6: the
    rows that pass writes on the main stream are read on the towers' streams - without record_stream the single graph reused
    their memory early and the input projections' dW came out as NaN) and steps like the tower-graph form.  The self-check
    itself: gradients tensor by tensor against the eager step's (a sign flip of a rounding-noise gradient under BertAdam must not
    fail it - it did at step 2 of bf16 runs); a replay whose gradient for ONE small tensor is wrong is rejected and the eager
    step's result stands."""
    import synth
    from dldkd_amd import ops
    from dldkd_amd import train as T
    from dldkd_amd.model import DLDKD
    from dldkd_amd.optimization import BertAdam
    cfg = types.SimpleNamespace(visual_input_size=3072, query_input_size=768, inheritance_hidden=384, exploration_hidden=384,
                                max_ctx_l=128, max_desc_l=30, input_drop=0.2, drop=0.2, n_heads=4, initializer_range=0.02,
                                margin=0.1, use_hard_negative=True, hard_pool_size=20, label_style="soft")
    mopt = types.SimpleNamespace(double_branch=True, kl_intra_weight=0.1, inher_nce_weight=0.04, explore_nce_weight=0.04,
                                 collection="tvr", alpha=0.8, belta=0.8)
    batch = synth.make_train_batch(3, nv=128, caps=5, L=128, len_lo=24, dv=3072, dq=768)
    batch = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}

    def make(par):
        torch.manual_seed(0)
        m = DLDKD(types.SimpleNamespace(**vars(cfg)), mopt).to(DEV).train()
        o = BertAdam([{"params": list(m.parameters()), "weight_decay": 0.01}], lr=3e-4, warmup=0.01, t_total=400)
        return m, o, T.GraphedTrainStep(m, o, types.SimpleNamespace(grad_clip=-1, parallel_tower_graphs=par))

    ops.set_gemm_precision(prec)
    try:
        res = {}
        for par in (True, False):
            m, o, g = make(par)
            torch.manual_seed(7)
            losses = [float(g(batch)[0]) for _ in range(4)]
            assert g.captures == 1 and g.fallbacks == [] and g.replays == 3, (par, g.fallbacks)
            assert g.last_check["finite"] and g.last_check["worst_grad_rel_l2"] < 1e-3 and g.last_check["d_loss"] < 1e-4, g.last_check
            assert bool(torch.isfinite(o.fp.flat).all())
            res[par] = (losses, o.fp.flat.clone())
        assert res[True][0] == pytest.approx(res[False][0], rel=2e-3)
        # a replay with ONE wrong gradient tensor (the position embedding's LayerNorm bias scaled by 1.5 behind the replay)
        m, o, g = make(True)
        idx = [n for n, _ in m.named_parameters()].index("visual_pos_embed.LayerNorm.bias")
        orig = T.GraphedTrainStep._replay
        state = {"armed": True}

        def bad_replay(self, e, b, staged=False):
            out = orig(self, e, b, staged)
            if state["armed"]:
                state["armed"] = False
                self.optimizer.fp.views()[idx].mul_(1.5)
            return out
        monkeypatch.setattr(T.GraphedTrainStep, "_replay", bad_replay)
        torch.manual_seed(7)
        l0 = float(g(batch)[0])                           # first sight: eager
        before = o.fp.flat.clone()
        l1 = float(g(batch)[0])                           # capture + check: rejected
        assert g.check_failures == 1 and g.captures == 0 and len(g.fallbacks) == 1 and "gradient" in g.fallbacks[0][0], g.fallbacks
        assert 0.3 < g.last_check["worst_grad_rel_l2"] < 0.7 and np.isfinite(l1) and not torch.equal(before, o.fp.flat)
        l2 = float(g(batch)[0])                           # the next notch (single graph) captures cleanly
        assert g.captures == 1 and np.isfinite(l2) and l0 > 0
    finally:
        ops.set_gemm_precision("fp32")


def test_memset_node_probe_selects_the_zeroing_mode_by_evidence():
    """staging.memset_node_defect: one memset node over the 296-byte buffer that showed the defect, replayed on an idle stream over a
    poisoned buffer; the native zeroing mode follows the result (defect -> kernel fills, clean -> memset nodes), and the replayed
    BertAdam step with gradient clipping - the consumer of that scratch buffer - equals the eager one in either mode."""
    from dldkd_amd import native, staging
    lib = native.lib()
    staging._MEMSET_PROBE.clear()
    seen = []
    lib.dldkd_set_zero_by_memset(0)
    defect = staging.memset_node_defect(torch.device(DEV), log=seen.append)
    assert len(seen) == 1 and "memset-node probe" in seen[0] and isinstance(defect, bool)
    print("  " + seen[0])
    assert lib.dldkd_set_zero_by_memset(0) == 0                           # logging only: the default keeps the kernel fill
    assert staging.memset_node_defect(torch.device(DEV), select=True) == defect and len(seen) == 1     # cached; now it selects
    assert lib.dldkd_set_zero_by_memset(0) == (0 if defect else 1)
    x = torch.full((1000,), 3.0, device=DEV)
    for mode in (0, 1):                                                   # the zeroing entry point itself, eager, both modes
        lib.dldkd_set_zero_by_memset(mode)
        x.fill_(3.0)
        native.check(lib.dldkd_zero_scratch_f32(native.ptr(x), 999, native.stream()), "zero")
        torch.cuda.synchronize()
        assert float(x[:999].abs().sum()) == 0.0 and float(x[999]) == 3.0
    # the optimizer entry point in both modes: per-tensor clipping of a flat gradient, eager launches (no graph: the mode only
    # changes HOW the scratch is zeroed)
    from dldkd_amd import optimization as optim
    torch.manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(n, device=DEV)) for n in (300, 5, 4097)]
    res = []
    for mode in (0, 1):
        lib.dldkd_set_zero_by_memset(mode)
        qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
        o = optim.BertAdam(qs, lr=1e-2, warmup=0.1, t_total=10, weight_decay=0.01, max_grad_norm=1.0)
        for it in range(3):
            for q in qs:
                q.grad = torch.full_like(q, 0.5 + it)
            o.step()
        torch.cuda.synchronize()
        res.append([q.detach().clone() for q in qs])
    lib.dldkd_set_zero_by_memset(0)
    for a, b in zip(*res):
        assert torch.equal(a, b)
