"""GPU: dh3d_match_descriptors2 (dh3d_amd.registration.match_descriptors2 -> csrc/match.hip) against its numpy restatement
(tests/match2_reference.py), bit for bit: the two nearest ids and distances, the reverse ids, the ratio / mutual mask and
its count; nn1 / dist1 against the plain matcher's kernel; adversarial inputs on which the MFMA screen excludes nothing;
batch independence, graph capture, poisoned allocations, and register(match=...)."""
import numpy as np
import pytest
import torch

import match2_reference as m2
from poisoned_alloc import KINDS, poisoned

pytestmark = pytest.mark.gpu

F = np.float32


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def _rows(desc):
    """[P, M, D] descriptors as keypoint rows hold them, [xyz | desc | score]: 132 columns wide up to D = 128."""
    P, M, D = desc.shape
    rows = np.full((P, M, max(132, 3 + D + 1)), 7.0, F)
    rows[:, :, 3:3 + D] = desc
    return rows


def _call(dev, a, b, ca, cb, **kw):
    """match_descriptors2 and match_descriptors on column views of the rows; everything back as numpy."""
    from dh3d_amd import registration as reg
    D = a.shape[2]
    ra, rb = torch.from_numpy(_rows(a)).to(dev), torch.from_numpy(_rows(b)).to(dev)
    ca, cb = (torch.tensor(list(c), dtype=torch.int32, device=dev) for c in (ca, cb))
    va, vb = ra[:, :, 3:3 + D], rb[:, :, 3:3 + D]
    assert va.stride(1) >= 132 and not va.is_contiguous()
    out = reg.match_descriptors2(va, ca, vb, cb, **kw)
    plain = reg.match_descriptors(va, ca, vb, cb)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["plain_match"], out["plain_dist"] = plain[0].cpu().numpy(), plain[1].cpu().numpy()
    return out


def _check_pair(out, p, a, b, na, nb, ratio=None, mutual=False, S=None):
    exp = m2.match2(a, b, na, nb, ratio=ratio, mutual=mutual, S=S)
    for k in ("nn1", "nn2", "match") + (("rev",) if mutual else ()):
        assert (out[k][p] == exp[k]).all(), (p, k, int((out[k][p] != exp[k]).sum()))
    for k in ("dist1", "dist2") + (("rev_dist",) if mutual else ()):
        assert (_bits(out[k][p]) == _bits(exp[k])).all(), (p, k)
    assert out["num_kept"][p] == exp["num_kept"], (p, out["num_kept"][p], exp["num_kept"])
    assert (out["nn1"][p] == out["plain_match"][p]).all() and (_bits(out["dist1"][p]) == _bits(out["plain_dist"][p])).all(), p
    return exp


SHAPES = [(1, 1), (3, 2), (31, 33), (257, 700), (700, 37), (40, 0), (0, 50)]


def _shape_batch(rng, D, shapes, M=700):
    """One pair per (na, nb) in [len(shapes), M, D] arrays; a share of the positives are noisy copies of anchors, and rows
    behind the counts hold descriptors that would win if they were read."""
    P = len(shapes)
    a, b = np.stack([m2.unit(rng, M, D) for _ in range(P)]), np.stack([m2.unit(rng, M, D) for _ in range(P)])
    for p, (na, nb) in enumerate(shapes):
        n = min(na, nb) // 2
        b[p, :n] = a[p, :n][::-1] + (0.05 * rng.standard_normal((n, D))).astype(F)
        if na < M:
            a[p, na:] = b[p, 0]
        if nb < M:
            b[p, nb:] = a[p, 0]
    return a, b


def test_every_output_against_the_restatement_d128(dev):
    a, b = _shape_batch(np.random.default_rng(0), 128, SHAPES)
    ca, cb = [s[0] for s in SHAPES], [s[1] for s in SHAPES]
    out = _call(dev, a, b, ca, cb, ratio=0.9, mutual=True)
    for p, (na, nb) in enumerate(SHAPES):
        exp = _check_pair(out, p, a[p], b[p], na, nb, ratio=0.9, mutual=True)
        assert (out["nn1"][p, na:] == -1).all() and np.isinf(out["dist2"][p, na:]).all() and (out["rev"][p, nb:] == -1).all()
        if min(na, nb) >= 30:
            assert 0 < exp["num_kept"] < na


@pytest.mark.parametrize("D", [4, 36, 256])
def test_other_descriptor_lengths(dev, D):
    a, b = _shape_batch(np.random.default_rng(D), D, [(257, 700)])
    out = _call(dev, a, b, [257], [700], ratio=0.9, mutual=True)
    _check_pair(out, 0, a[0], b[0], 257, 700, ratio=0.9, mutual=True)


def test_full_size_pair(dev):
    rng = np.random.default_rng(2)
    M, D = 4096, 128
    a, b = m2.unit(rng, M, D), m2.unit(rng, M, D)
    b[:1500] = a[1000:2500] + (0.05 * rng.standard_normal((1500, D))).astype(F)
    out = _call(dev, a[None], b[None], [M], [M], ratio=0.9, mutual=True)
    exp = _check_pair(out, 0, a, b, M, M, ratio=0.9, mutual=True)
    assert 1000 < exp["num_kept"] < 2000


def test_adversarial_pairs(dev):
    """Duplicated positives, anchors equal to a positive, neighbours one ulp apart in S, rows sharing a large offset, all
    rows equal: the screen separates little or nothing here, the rule decides every pair."""
    rng = np.random.default_rng(4)
    cases = [("duplicates", m2.with_duplicates(rng, 200, 128)), ("one ulp apart", m2.ulp_neighbours(rng, 200, 36)),
             ("shared offset", m2.shared_offset(rng, 300, 128)), ("all equal", m2.all_equal(130, 36)),
             ("all equal D=256", m2.all_equal(130, 256))]
    for name, (a, b) in cases:
        M = len(a)
        for kw in (dict(ratio=1.0, mutual=True), dict()):
            out = _call(dev, a[None], b[None], [M], [M], **kw)
            exp = _check_pair(out, 0, a, b, M, M, **kw)
            if name.startswith("all equal") and kw:
                assert exp["num_kept"] == 0 and (out["nn2"][0] == 1).all() and (out["dist2"][0] == 0).all(), name
    a, b = cases[0][1]
    out = _call(dev, a[None], b[None], [200], [200])
    assert out["nn1"][0, :4].tolist() == [5, 20, 20, 7] and out["nn2"][0, :3].tolist() == [9, 21, 21]


def test_ratio_and_mutual_alone_and_together(dev):
    from dh3d_amd import registration as reg
    rows_a, rows_b, truth, _ = m2.planted(P=2)
    a, b = rows_a[:, :, 3:131], rows_b[:, :, 3:131]
    S = [m2.rule_sums(a[p], b[p]) for p in range(2)]
    kept = {}
    for name, kw in (("none", dict()), ("ratio", dict(ratio=0.9)), ("mutual", dict(mutual=True)),
                     ("both", dict(ratio=0.9, mutual=True)), ("ratio 1", dict(ratio=1.0))):
        out = _call(dev, a, b, [512, 300], [512, 512], **kw)
        assert ("rev" in out) == bool(kw.get("mutual"))
        for p, na in enumerate((512, 300)):
            _check_pair(out, p, a[p], b[p], na, 512, S=S[p][:na], **kw)
        kept[name] = out["num_kept"].tolist()
    assert kept["none"] == [512, 300] and kept["ratio 1"] == [512, 300]          # no exact ties among random rows
    assert all(kept["both"][p] <= min(kept["ratio"][p], kept["mutual"][p]) < kept["none"][p] for p in range(2))
    t = torch.zeros(1, 8, 128, device=dev)
    c = torch.full((1,), 8, dtype=torch.int32, device=dev)
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError):
            reg.match_descriptors2(t, c, t, c, ratio=bad)


def _equal_dicts(x, y, where):
    assert set(x) == set(y), where
    for k, v in x.items():
        w = y[k]
        if v.dtype == torch.float64:
            assert torch.equal(v.view(torch.int64), w.view(torch.int64)), (where, k)  # (bit for bit, NaN included)
        elif v.dtype == torch.float32:
            assert torch.equal(v.view(torch.int32), w.view(torch.int32)), (where, k)
        else:
            assert torch.equal(v, w), (where, k)


def test_batch_independence(dev):
    from dh3d_amd import registration as reg
    P = 6
    rows_a, rows_b, _, _ = m2.planted(seed=12, P=P, M=200)
    A, B = torch.from_numpy(rows_a).to(dev)[:, :, 3:131], torch.from_numpy(rows_b).to(dev)[:, :, 3:131]
    CA = torch.tensor([200, 0, 1, 65, 200, 130], dtype=torch.int32, device=dev)
    CB = torch.tensor([200, 50, 200, 1, 0, 64], dtype=torch.int32, device=dev)
    full = reg.match_descriptors2(A, CA, B, CB, ratio=0.9, mutual=True)
    for p in range(P):
        one = reg.match_descriptors2(A[p:p + 1], CA[p:p + 1], B[p:p + 1], CB[p:p + 1], ratio=0.9, mutual=True)
        _equal_dicts(one, {k: v[p:p + 1] for k, v in full.items()}, p)
    assert int(full["num_kept"][0]) > 50


def test_graph_capture_replays_on_new_inputs(dev):
    from dh3d_amd import registration as reg
    P, M = 4, 300
    ra, rb, _, _ = m2.planted(seed=20, P=P, M=M)
    sa, sb = torch.from_numpy(ra).to(dev), torch.from_numpy(rb).to(dev)
    sca = torch.full((P,), M, dtype=torch.int32, device=dev)
    scb = sca.clone()
    run = lambda a, ca, b, cb: reg.match_descriptors2(a[:, :, 3:131], ca, b[:, :, 3:131], cb, ratio=0.9, mutual=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(sa, sca, sb, scb)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gout = run(sa, sca, sb, scb)
    for seed in (21, 22):
        na, nb, _, _ = m2.planted(seed=seed, P=P, M=M)
        r = np.random.default_rng(seed)
        ca = torch.from_numpy(r.integers(M // 2, M + 1, P).astype(np.int32)).to(dev)
        cb = torch.from_numpy(r.integers(M // 2, M + 1, P).astype(np.int32)).to(dev)
        a, b = torch.from_numpy(na).to(dev), torch.from_numpy(nb).to(dev)
        sa.copy_(a)
        sb.copy_(b)
        sca.copy_(ca)
        scb.copy_(cb)
        g.replay()
        eout = run(a, ca, b, cb)
        torch.cuda.synchronize()
        _equal_dicts(eout, gout, seed)
        assert 0 < int(eout["num_kept"].sum()) < int(ca.sum())


def test_poisoned_allocations_change_nothing(dev):
    from dh3d_amd import registration as reg
    rows_a, rows_b, _, _ = m2.planted(seed=30, P=3, M=200)
    A, B = torch.from_numpy(rows_a).to(dev), torch.from_numpy(rows_b).to(dev)
    CA = torch.tensor([200, 70, 0], dtype=torch.int32, device=dev)
    CB = torch.tensor([130, 200, 9], dtype=torch.int32, device=dev)
    runs = {}
    for kind in (None,) + KINDS:
        with poisoned(kind):
            runs[kind] = (reg.match_descriptors2(A[:, :, 3:131], CA, B[:, :, 3:131], CB, ratio=0.9, mutual=True),
                          reg.register(A, CA, B, CB, match={"ratio": 0.9, "mutual": True}, seed=5))
        torch.cuda.synchronize()
    for kind in KINDS:
        _equal_dicts(runs[kind][0], runs[None][0], kind)
        _equal_dicts(runs[kind][1], runs[None][1], kind)


def test_register_with_match_options(dev):
    from dh3d_amd import registration as reg
    P, M = 4, 512
    rows_a, rows_b, truth, T = m2.planted(P=P)
    A, B = torch.from_numpy(rows_a).to(dev), torch.from_numpy(rows_b).to(dev)
    cnt = torch.full((P,), M, dtype=torch.int32, device=dev)
    opts = {"ratio": 0.9, "mutual": True}
    res = reg.register(A, cnt, B, cnt, match=opts, seed=3)
    mm = reg.match_descriptors2(A[:, :, 3:131], cnt, B[:, :, 3:131], cnt, **opts)
    fit = reg.ransac_rigid(A, B, mm["match"], cnt, seed=3)
    _equal_dicts(res, dict(fit, dist=mm["dist1"], **mm), "register(match=opts)")
    # the restatement's mask, and the pose it leads to
    for p in range(P):
        exp = m2.match2(rows_a[p, :, 3:131], rows_b[p, :, 3:131], M, M, **opts)
        assert (res["match"][p].cpu().numpy() == exp["match"]).all(), p
    assert (res["num_corr"] == res["num_kept"]).all() and bool(res["valid"].all())
    dt, dd = reg.transform_errors(T, res["Rt"], res["valid"])
    assert (dt < 0.1).all() and (dd < 1.0).all(), (dt.max(), dd.max())
    plain = reg.register(A, cnt, B, cnt, seed=3)
    assert (res["inlier_ratio"] > plain["inlier_ratio"]).all() and (res["trials"] <= plain["trials"]).all()
    # {}: the new entry without a filter is the plain matcher's list, so the same fit
    none = reg.register(A, cnt, B, cnt, match={}, seed=3)
    assert "rev" not in none and (none["num_kept"] == M).all()
    for k in plain:
        _equal_dicts({k: none[k]}, {k: plain[k]}, "match={} " + k)
    # match=None is today's call: match_descriptors, then ransac_rigid, and nothing else in the result
    m, d = reg.match_descriptors(A[:, :, 3:131], cnt, B[:, :, 3:131], cnt)
    _equal_dicts(plain, dict(reg.ransac_rigid(A, B, m, cnt, seed=3), match=m, dist=d), "register(match=None)")
    _equal_dicts(reg.register(A, cnt, B, cnt, match=None, seed=3), plain, "match=None")
    # too few correspondences after the filters: not valid, as without them
    few = reg.register(A, torch.full((P,), 2, dtype=torch.int32, device=dev), B, cnt, match=opts)
    assert not bool(few["valid"].any()) and bool(torch.isnan(few["Rt"]).all())
