"""GPU: the stage 1-2 training step (dh3d_amd.training.LocalTrainer; core/model.py:135-246 with basic_config /
detection_config, core/losses.py:29-133) -- the WHOLE local backbone (and the detector) in training mode, forward and
backward on HIP kernels.

  * forward against the oracle's training-mode graph (oracle/model_np.local_training_step_forward): loss, descriptors,
    every moving average the step updates, at 2 x (anchor + positive) x 4096 points;
  * gradients of every trainable tensor against a float64 torch restatement of the same graph (gather-based flex_conv /
    conv_pointset / flex_pool written with tensor ops, autograd's gradients);
  * the captured whole-step hipGraph follows eager steps; a short run reduces the loss.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PAIRS, N, M = 2, 4096, 256
# f32 kernels (bf16x6 / exact-f32 GEMMs, f32 atomics in the scatters) against a float64 graph through ~20 layers with ten
# BatchNorm backward passes, the float64 side on the kernels' ReLU patterns and pooling argmaxes: measured worst 7.6e-4
# (biases in front of a BatchNorm, rounding noise against the floor, 4 x 4096 and 6 x 3000 alike).  Deciding the
# patterns in float64 instead gave 3.2e-3 at 4 x 4096 and 2e-2 at 6 x 3000: kinks within rounding of 0
TOL_GRAD = 3e-3


def _weights_np(model):
    from dh3d_amd.model import tf_variable_name
    return {tf_variable_name(k): v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}


def _build(dev, preset, seed=5, n=N, pairs=PAIRS):
    from dh3d_amd import ConfigFactory
    from dh3d_amd.model import DH3D
    cfg = ConfigFactory(preset).getconfig()
    cfg.num_points, cfg.batch_size, cfg.sampled_kpnum = n, pairs, M
    m = DH3D(cfg).init_synthetic(seed)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, buf in m.named_buffers():
            if name.endswith("mean_EMA"):
                buf.copy_(0.1 * torch.randn(buf.shape, generator=g))
            elif name.endswith("variance_EMA"):
                buf.copy_(0.5 + torch.rand(buf.shape, generator=g))
        for name, p in m.named_parameters():
            if name.endswith("gamma"):
                p.copy_(0.75 + 0.5 * torch.rand(p.shape, generator=g))
    return m.to(dev).eval().prepare()


def _pairs(seed=77, n=N, pairs=PAIRS, m=M, extent=12.0):
    """Registered cloud pairs: positive = anchor @ R + jitter in the SAME point order; half of the positive's keypoints
    are the anchor's (true correspondences), half are drawn independently (negatives within the search radius)."""
    rng = np.random.default_rng(seed)
    anc = (rng.random((pairs, n, 3), dtype=np.float32) * extent).astype(np.float32)
    Rm = np.zeros((pairs, 3, 3), np.float32)
    for b in range(pairs):
        a = rng.uniform(0, 2 * np.pi)
        Rm[b] = np.array([[np.cos(a), np.sin(a), 0], [-np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float32)
    pos = (np.matmul(anc, Rm) + rng.normal(0, 0.02, anc.shape)).astype(np.float32)
    ia = np.stack([rng.permutation(n)[:m] for _ in range(pairs)]).astype(np.int32)
    ip = ia.copy()
    ip[:, m // 2:] = np.stack([rng.permutation(n)[: m - m // 2] for _ in range(pairs)])
    return np.concatenate([anc, pos]), Rm, np.concatenate([ia, ip])


def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("preset", ["basic_config", "detection_config"])
def test_local_training_forward_vs_oracle(dev, preset):
    from dh3d_amd.training import LocalTrainer
    from oracle import model_np
    m = _build(dev, preset)
    pts, Rm, idx = _pairs()
    w0 = _weights_np(m)
    exp_loss, exp, upd = model_np.local_training_step_forward(pts, Rm, idx, w0, dict(m.config))
    tr = LocalTrainer(m, graph_step=False)
    tr.keep_grads = True
    loss = tr.forward_loss(_T(pts, dev), _T(Rm, dev), _T(idx, dev))
    outs = tr.last_outs
    torch.cuda.synchronize()
    feat = outs["feat"].detach().cpu().numpy()
    scale = float(np.abs(exp["feat"]).max())
    assert np.abs(feat - exp["feat"]).max() <= 1e-4 * scale + 1e-5, np.abs(feat - exp["feat"]).max() / scale
    assert np.abs(outs["local_desc"].detach().cpu().numpy() - exp["local_desc"]).max() <= 1e-4
    assert np.array_equal(outs["xyz_sampled"].cpu().numpy(), exp["xyz_sampled"])
    assert np.abs(outs["feat_sampled"].detach().cpu().numpy() - exp["feat_sampled"]).max() <= 1e-4
    if m.config.detection:
        assert np.abs(outs["attention"].detach().cpu().numpy() - exp["attention"]).max() <= 1e-4
    assert abs(float(loss) - exp_loss) <= 1e-4 * max(1.0, abs(exp_loss)), (float(loss), exp_loss)
    assert exp_loss > 0.05  # positives and negatives both present: a loss that means something
    from dh3d_amd.model import tf_variable_name
    sd = {tf_variable_name(k): v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    assert len(upd) == (22 if m.config.detection else 16), sorted(upd)
    for name, e in upd.items():
        assert not np.array_equal(sd[name], w0[name]), name  # it moved
        assert np.allclose(sd[name], e, rtol=1e-4, atol=1e-6), (name, np.abs(sd[name] - e).max())


# ---------------------------------------------------------------------------------------- float64 torch restatement
def _gather(x, nbr):  # x [B,N,C], nbr [B,N,K] -> [B,N,K,C]
    B, Nn, K = nbr.shape
    return torch.gather(x.unsqueeze(1).expand(B, Nn, x.shape[1], x.shape[2]), 2,
                        nbr.long().unsqueeze(-1).expand(B, Nn, K, x.shape[2]))


def _bn_t(x, bn, eps):  # batch statistics over all rows, biased variance (training mode)
    mu = x.mean((0, 1), keepdim=True)
    var = ((x - mu) ** 2).mean((0, 1), keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * bn.gamma.double() + bn.beta.double()


def _flex_t(x, xyz, nbr, fc):
    fn = _gather(x, nbr)                                                         # [B,N,K,Din]
    dp = _gather(xyz, nbr) - xyz.unsqueeze(2)                                    # [B,N,K,3]
    out = fn.sum(2) @ fc.position_bias.double()
    for d in range(3):
        out = out + (dp[..., d:d + 1] * fn).sum(2) @ fc.position_theta[d].double()
    return out + fc.feature_bias.double().reshape(1, 1, -1)


def _stack_t(mod, x, xyz, nbr, pat, i):
    for j in range(len(mod.outdims)):
        fc, bn = getattr(mod, "flexconv_%d" % j), getattr(mod, "flexconv_%d_bn" % j)
        x = pat.bn_relu(_bn_t(_flex_t(x, xyz, nbr, fc), bn, bn.eps), bn)
    pool = pat.flex_pool(x, nbr, i + 1)
    f1, f2 = mod.se.f1.tfconv0, mod.se.f2.tfconv0
    sq = pat.squeeze_relu(pool @ f1.W.double().reshape(f1.cin, f1.cout) + f1.b.double(), i)
    g = torch.sigmoid(sq @ f2.W.double().reshape(f2.cin, f2.cout) + f2.b.double())
    return pat.se_gate(x + x * g, i)


def _conv_t(x, fc1d, pat):
    c = fc1d.tfconv0
    return pat.bn_relu(_bn_t(x @ c.W.double().reshape(c.cin, c.cout) + c.b.double(), c.bn, c.bn.eps), c.bn)


def _restated_loss(m, pts, R, idx, lv, nbr, pat):
    """The same graph in float64 tensor ops (integer geometry taken from the HIP forward: it is exact).  Every ReLU mask
    and flex_pool argmax is the one the HIP forward took (pat: local_training_reference.ActivationPatterns, recorded
    during that forward): where a float32 pre-activation lies within rounding of 0, float64 deciding for itself would
    move a whole dy to the other side -- with four such entries on the detector's 1024-wide layer the feat gradient
    moved by 3e-2 (a shape-dependent lottery)."""
    from dh3d_amd import losses
    xyz = pts.double()
    dp = _gather(xyz, nbr) - _gather(xyz, nbr)[:, :, 0:1]
    ic = m.initconv
    init = dp.sum(2) @ ic.position_theta.double() + ic.position_bias.double()
    init = pat.bn_relu(_bn_t(init, m.initconv_bn, m.initconv_bn.eps), m.initconv_bn)
    init = pat.flex_pool(init, nbr, 0)
    x1 = _stack_t(m.stage1, init, xyz, nbr, pat, 0)
    x2 = _conv_t(x1, m.before_stage2_conv1d, pat)
    idxs = lv["idx"].long()
    fs = torch.gather(x2, 1, idxs.unsqueeze(-1).expand(-1, -1, x2.shape[2]))
    y = _stack_t(m.stage2, fs, lv["xyz_s"].double(), lv["nbr_s"], pat, 1)
    d = torch.clamp(lv["nn3_dist"].double(), min=1e-10)
    wts = (1.0 / d) / (1.0 / d).sum(2, keepdim=True)
    up = (_gather(y, lv["nn3_idx"]) * wts.unsqueeze(-1)).sum(2)
    x2 = _conv_t(torch.cat([up, x2], 2), m.stage2.concat_conv1d, pat)
    feat = _conv_t(x1, m.local_stage1_shortcut, pat) + x2
    desc = feat * torch.rsqrt(torch.clamp((feat * feat).sum(2, keepdim=True), min=1e-8))
    kp = idx.long()
    take = lambda t: torch.gather(t, 1, kp.unsqueeze(-1).expand(-1, -1, t.shape[2]))
    # (coordinates stay float32: the losses' masks -- which pairs count as positives / negatives -- are then the very
    #  same booleans the HIP step computed)
    outs = {"xyz": pts, "feat": feat, "local_desc": desc, "R": R, "sample_nodes_concat": idx.reshape(idx.shape[0], -1, 1),
            "xyz_sampled": take(pts), "feat_sampled": take(desc)}
    if m.config.detection:
        det = m.detection_block_reliable
        x = feat
        last = len(det.conv_dims) - 1
        for i in range(last + 1):
            c = getattr(det, "detec_conv%d" % i)
            pre = _bn_t(x @ c.W.double().reshape(c.cin, c.cout) + c.b.double(), c.bn, c.bn.eps)
            x = pat.head_relu(pre) if i == last else pat.bn_relu(pre, c.bn)
        fcw = det.detec_conv_fc
        att = torch.sigmoid(x @ fcw.W.double().reshape(-1, 1) + fcw.b.double())
        outs["attention"], outs["att_sampled"] = att, take(att)
    return losses.compute_loss(outs, m.config)


@pytest.mark.parametrize("preset", ["basic_config", "detection_config"])
def test_local_training_gradients_vs_float64_restatement(dev, preset, monkeypatch):
    _gradients_vs_float64(dev, preset, PAIRS, N, monkeypatch)


@pytest.mark.parametrize("preset", ["basic_config", "detection_config"])
def test_local_training_gradients_vs_float64_restatement_ragged(dev, preset, monkeypatch):
    """3 pairs x 3000 points: B*N = 18000 rows (not a multiple of 64 or 256), the dilate-8 level 375 points per cloud."""
    _gradients_vs_float64(dev, preset, 3, 3000, monkeypatch)


def _gradients_vs_float64(dev, preset, pairs, n, monkeypatch):
    import local_training_reference as LR
    from dh3d_amd.training import LocalTrainer, local_trainable_parameters
    pts, Rm, idx = _pairs(seed=78, n=n, pairs=pairs)
    tp, tR, ti = _T(pts, dev), _T(Rm, dev), _T(idx, dev)
    m = _build(dev, preset, seed=6, n=n, pairs=pairs)
    names = {id(p): n for n, p in m.named_parameters()}
    tr = LocalTrainer(m, graph_step=False, weight_decay=0.0)
    pat = LR.ActivationPatterns(monkeypatch)
    loss = tr.forward_loss(tp, tR, ti)
    monkeypatch.undo()
    loss.backward()
    params = local_trainable_parameters(m)
    got = [(names[id(p)], p.grad.detach().double().clone()) for p in params if p.grad is not None]
    for p in params:
        p.grad = None
    with torch.no_grad():
        geo = m._geometry(tp, None)
        m._join_side(geo)
        lv = geo.level(8, 8)
        nbr = geo.nbr
    ref = _restated_loss(m, tp, tR, ti, lv, nbr, pat)
    assert abs(float(ref) - float(loss)) <= 1e-4 * max(1.0, abs(float(ref))), (float(ref), float(loss))
    ref.backward()
    exp = {names[id(p)]: p.grad.detach().double().clone() for p in params if p.grad is not None}
    assert len(got) == len(exp) >= (34 if preset == "basic_config" else 44), (len(got), len(exp))
    top = max(float(v.abs().max()) for v in exp.values())
    report = []
    for k, a in got:
        b = exp[k]
        # (biases in front of a BatchNorm have an exactly-zero gradient: the floor keeps them from being compared
        #  relative to their own rounding noise)
        scale = max(float(b.abs().max()), 1e-4 * top)
        err = float((a - b).abs().max()) / scale
        report.append((err, k, scale / top))
    print("local training gradient errors at %d x %d (relative to the tensor's largest entry; tensor scale / largest "
          "gradient):" % (2 * pairs, n), [(round(e, 5), k, round(r, 5)) for e, k, r in sorted(report, reverse=True)[:8]],
          "loss |diff| %.3g, kinks where float64 would have gone the other way: %d" % (abs(float(ref) - float(loss)),
                                                                                  pat.flips))
    for err, k, _ in report:
        assert err <= TOL_GRAD, (k, err)


def test_local_trainer_whole_step_graph_follows_eager_steps_and_learns(dev):
    from dh3d_amd.training import LocalTrainer
    batches = [tuple(_T(a, dev) for a in _pairs(seed=s, n=2048, m=128)) for s in (90, 91)]
    traj = []
    for graph in (True, False):
        m = _build(dev, "detection_config", seed=9)
        tr = LocalTrainer(m, start_lr=2e-4, graph_step=graph)
        ls = [tr.step(*batches[i % 2]) for i in range(8)]
        assert bool(tr._graphs) == graph
        traj.append(ls)
    assert all(np.isfinite(traj[0])) and all(np.isfinite(traj[1]))
    for x, y in zip(*traj):
        assert abs(x - y) <= 3e-2 * max(1.0, abs(y)), traj
    # a longer run on one batch: the descriptors of corresponding keypoints move together
    m = _build(dev, "basic_config", seed=10)
    tr = LocalTrainer(m, start_lr=1e-3)
    ls = [tr.step(*batches[0]) for _ in range(40)]
    assert np.mean(ls[-5:]) < 0.8 * np.mean(ls[:5]), (ls[:5], ls[-5:])
    # the inference path sees the trained weights and moving averages
    m.eval()
    with torch.no_grad():
        o = m(batches[0][0], fetch=("xyz_feat",))
    assert torch.isfinite(o["xyz_feat"]).all()


# ------------------------------------------------------------------------------- the captured step, gradient by gradient
# Graphed replays against eager steps of a twin trainer.  At start_lr = 1e-8 the two trajectories stay the same up to
# the order of the f32 atomics (see test_trainer_zero_arena_and_input_buffer in test_training_gpu.py), so each step's
# gradients can be compared, relative to each tensor's largest entry (floored at 1e-4 of the largest gradient, as above):
# measured worst 1.3e-3 (detec_conv2.W at one replay, a ReLU kink taken differently; 4.9e-4 in other runs), compared as
# _grad_errors says.
# A doubled gradient is off by 1, a stale accumulator (not re-zeroed in a replay) by ~1.
TOL_REPLAY = TOL_GRAD
# the two trainers' losses, relative: measured worst 1.2e-7 (two captured shapes)
TOL_LOSS = 1e-5
# BatchNorm moving averages after the last step, relative to each buffer's largest entry: measured worst 1.5e-7
TOL_EMA = 1e-5


def _grad_errors(trainer, got, want):
    names = {id(p): n for n, p in trainer.model.named_parameters()}
    assert len(got) == len(want) == len(trainer.params)
    top = max(float(w.abs().max()) for w in want if w is not None)
    worst = (-1.0, "")
    for p, a, b in zip(trainer.params, got, want):
        assert (a is None) == (b is None), names[id(p)]
        if b is None:
            continue
        n = names[id(p)]
        # a bias in front of a BatchNorm has an exact gradient of 0: both runs hold column sums of rounding noise, which
        # the atomics' order changes (measured up to 2.5e-5 of the largest gradient, on the detector's) -- compared
        # against the largest gradient.  The others against their own largest entry, floored at 0.1 of the largest
        # gradient: two float32 runs sum their atomics in different orders, so a pre-activation within an ulp of a
        # ReLU kink can land on either side and move a whole dy (measured: 8.6e-3 of detec_conv2.W's own largest
        # entry, 1.3e-4 of the largest gradient, at one replay).  A doubled or stale gradient of any tensor larger
        # than 3e-2 x TOL_REPLAY of the largest still fails; the smallest trained tensor here is 5e-3 of it.
        zero = n.endswith("feature_bias") or n == "initconv.position_bias" or (
            n.endswith(".b") and n[:-2] + ".bn.gamma" in names.values())
        err = float((a - b).abs().max()) / (top if zero else max(float(b.abs().max()), 0.1 * top))
        worst = max(worst, (err, names[id(p)]))
    return worst


def _ema_error(ma, mb):
    bufs_b = dict(mb.named_buffers())
    worst = (-1.0, "")
    for name, a in ma.named_buffers():
        if name.endswith(("EMA", "moving_mean", "moving_variance")):
            b = bufs_b[name]
            worst = max(worst, (float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30), name))
    return worst


def _twins(dev, preset, seed, **kw):
    from dh3d_amd.training import LocalTrainer
    ma, mb = _build(dev, preset, seed=seed), _build(dev, preset, seed=seed)
    graphed = LocalTrainer(ma, graph_step=True, **kw)
    eager = LocalTrainer(mb, graph_step=False, **kw)
    eager.keep_grads = True
    return graphed, eager


def _step_both(graphed, eager, batch):
    la, lb = graphed.step(*batch), eager.step(*batch)
    got = [None if p.grad is None else p.grad.detach().clone() for p in graphed.params]
    assert abs(la - lb) <= TOL_LOSS * max(1.0, abs(lb)), (la, lb)
    return abs(la - lb), _grad_errors(graphed, got, eager.last_grads)


def test_local_trainer_graph_replays_match_eager_steps_gradient_by_gradient(dev):
    """Eight steps on alternating batches (three eager, then the capture and its replays), the learning-rate staircase
    crossed once (decay_step = 4: step 5 runs at half the rate): after every step each parameter's p.grad on the graphed trainer -- that replay's
    gradient -- against the eager twin's; the moving averages after the last step."""
    batches = [tuple(_T(a, dev) for a in _pairs(seed=s, n=2048, m=128)) for s in (92, 93)]
    graphed, eager = _twins(dev, "detection_config", 12, start_lr=1e-8, decay_step=4, decay_rate=0.5)
    report = []
    for i in range(8):
        dl, (err, name) = _step_both(graphed, eager, batches[i % 2])
        report.append((round(err, 6), name, "%.2g" % dl))
    assert len(graphed._graphs) == 1 and not eager._graphs
    assert graphed._lr_value == eager._lr_value == 1e-8 * 0.5 ** (7 // 4)
    ema = _ema_error(graphed.model, eager.model)
    print("graph replay vs eager: per-step worst gradient error", report, "moving averages", ema)
    for i, (err, name, _) in enumerate(report):
        assert err <= TOL_REPLAY, (i, name, err)
    assert ema[0] <= TOL_EMA, ema


def test_local_trainer_zero_arena_matches_torch_zeros(dev, monkeypatch):
    """The step's accumulators from ONE zeroed arena (pm.ZeroArena) against a torch.zeros each: the same gradients over
    two eager steps; the arena is in use and asks for the same bytes every step."""
    from dh3d_amd import pm
    from dh3d_amd.training import LocalTrainer
    batches = [tuple(_T(a, dev) for a in _pairs(seed=s, n=2048, m=128)) for s in (94, 95)]
    runs = []
    for arena in (True, False):
        if not arena:
            monkeypatch.setattr(pm.ZeroArena, "take",
                                lambda self, shape, dtype, device: torch.zeros(shape, dtype=dtype, device=device))
        m = _build(dev, "detection_config", seed=13)
        tr = LocalTrainer(m, start_lr=1e-8, graph_step=False)
        tr.keep_grads = True
        out = []
        for b in batches:
            out.append((tr.step(*b), [None if g is None else g.clone() for g in tr.last_grads]))
        if arena:   # (the first step records the demand, the second begin() sizes the buffer to it)
            assert tr._zarena.buf is not None and tr._zarena.off > 0
            assert tr._zarena.demand == tr._zarena.peak > 0    # the same requests every step
        runs.append((out, tr))
    monkeypatch.undo()
    (oa, tra), (ob, _) = runs
    report = []
    for (la, ga), (lb, gb) in zip(oa, ob):
        assert abs(la - lb) <= TOL_LOSS * max(1.0, abs(lb)), (la, lb)
        report.append(_grad_errors(tra, ga, gb) + ("%.2g" % abs(la - lb),))
    print("zero arena vs torch.zeros: worst gradient error per step", report)
    for err, name, _ in report:
        assert err <= TOL_REPLAY, (name, err)


def test_local_trainer_graphs_of_two_shapes_match_eager_steps(dev):
    """N = 2048 captured, then N = 4096 warmed up (the eager arena grows and frees its old buffer) and captured, then
    the two alternate with junk written into freed allocator memory between steps.  Both graphs stay captured with
    arenas of their own, and every step's gradients match an eager twin's.  (This test found p.grad still naming the
    OTHER shape's captured gradients after a replay: LocalTrainer.step now points p.grad at the replayed graph's.)"""
    small = [tuple(_T(a, dev) for a in _pairs(seed=s, n=2048, m=128)) for s in (96, 97)]
    large = [tuple(_T(a, dev) for a in _pairs(seed=s, n=4096, m=128)) for s in (98, 99)]
    order = [small[0]] * 4 + [large[0]] * 4 + [small[1], large[1], small[0], large[0]]
    graphed, eager = _twins(dev, "basic_config", 14, start_lr=1e-8)
    report = []
    for i, b in enumerate(order):
        dl, (err, name) = _step_both(graphed, eager, b)
        report.append((round(err, 6), name, "%.2g" % dl))
        if i >= 3:
            # scribble over whatever the caching allocator hands out now: a replay into freed memory would
            # accumulate onto this instead of onto zeros
            junk = torch.full((1 << 22,), 1e30, device=dev)
            del junk
    assert len(graphed._graphs) == 2, list(graphed._graphs)
    arenas = [ent[3] for ent in graphed._graphs.values()]
    assert all(a.fixed and a.buf is not None for a in arenas)
    assert arenas[0].buf.data_ptr() != arenas[1].buf.data_ptr()
    print("two captured shapes vs eager: per-step worst gradient error", report)
    for i, (err, name, _) in enumerate(report):
        assert err <= TOL_REPLAY, (i, name, err)
