"""No GPU: pins tests/netvlad_reference.py and proves that the cases of tests/test_netvlad_kernels_gpu.py can see what they
are meant to see.  On the very inputs the GPU file uses (the generators are shared):
  identities   fused with the whole-vector factor behind the projection = head(aggregate); tail_assign(walk) = fused on the
               materialised up-sampling (the commutation the kernels rely on); aggregate = oracle.model_np at f32 resolution;
  mutations    every mistake of MUTATIONS moves some element by ten bounds or more on every case listed for it, and the
               unmutated reference evaluated in float32 numpy stays under the bound on every case;
  degenerate   closed forms: zero attention -> vlad = 0, out = bn1_shift; a zero row adds att softmax(cl_shift) to asum."""
import functools

import numpy as np
import pytest

import dense_reference as D
import netvlad_reference as R

F32 = np.float32


def _ratio(got, ref, E):
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / E).max())


# ------------------------------------------------------------------------------------------------------- identities
def test_fused_with_tot_equals_head_of_aggregate():
    c = R.agg_case(2, 65)
    hp = R.head_params(R.seed("id"), R.DM * R.CL)
    for l2 in (0.0, 1e-8):
        a, _ = R.fused(*c, *hp, l2)
        b, _ = R.fused(*c, *hp, l2, use_tot=False)
        assert np.abs(a - b).max() <= 1e-14 * max(1.0, np.abs(a).max())


@pytest.mark.parametrize("shape", [(3, 127, 3, "nn", 256), (3, 300, 40, "nn", 256), (3, 300, 200, "random", 256)])
def test_walk_then_tail_equals_fused_on_upsampled(shape):
    case = R.walk_case(*shape)
    W_att, att_ep, w_fc, b_fc, Wc, sc, sh = case["par"]
    rng = R.seed("comm", shape)
    W2 = (rng.standard_normal((R.DM, R.CL)) / 16).astype(F32)
    hp = R.head_params(rng, R.DM * R.CL)
    att, _, apart, _, asum, _ = R.walk_ref(case)
    a, _ = R.tail_assign(apart, case["coarse"], asum, W2, *hp, 1e-8)
    up, _ = D.three_interpolate_idw(case["coarse"], case["idx"], case["dist"])
    att2 = D.interp_head(case["coarse"], case["idx"], case["dist"], W_att, w_fc, b_fc, att_ep)[0][..., 0]
    assert np.array_equal(att, att2)
    b, _ = R.fused(up, att2, Wc, sc, sh, W2, *hp, 1e-8)
    assert np.abs(a - b).max() <= 1e-12


def test_aggregate_agrees_with_oracle():
    from oracle import model_np
    x, att, Wc, sc, sh, W2 = R.agg_case(2, 200)
    rng = R.seed("oracle")
    hp = R.head_params(rng, R.DM * R.CL)
    w = {"cluster_weights": Wc, "cluster_weights2": W2[None], "hidden1_weights": hp[0], "gating_weights": hp[3]}
    for s, (scale, shift) in (("cluster_bn", (sc, sh)), ("bn", hp[1:3]), ("gating_bn", hp[4:6])):
        w[s + "/gamma"], w[s + "/beta"] = scale.astype(np.float64), shift
        w[s + "/moving_mean"] = np.zeros_like(shift)
        w[s + "/moving_variance"] = np.ones_like(shift, dtype=np.float64) - 1e-3      # gamma / sqrt(var + eps) = gamma
    exp = model_np.global_netvlad_block(x, att[..., None], w, 1e-3)
    got, _ = R.fused(x, att, Wc, sc, sh, W2, *hp, 0.0)
    assert np.abs(got - exp).max() <= 2e-5 * np.abs(exp).max()       # the oracle rounds to f32 at every stage


# -------------------------------------------------------------------------------------------------------- mutations
def _agg(case):
    return lambda **kw: R.aggregate(*case, **kw)


def _hd(case, l2):
    return lambda **kw: R.head(*case, l2, **kw)


def _wk(case):
    def run(**kw):
        r = R.walk_ref(case, **kw)
        return np.concatenate([r[2].reshape(-1), r[4].reshape(-1)]), np.concatenate([r[3].reshape(-1), r[5].reshape(-1)])
    return run


def _onehot_head(Kd, B=33):
    vlad, *par = R.head_case(Kd, B, gating=False)
    vlad[:] = 0
    vlad[np.arange(B), Kd - 1 - np.arange(B)] = 1.0          # the last B columns, one per row
    return (vlad,) + tuple(par)


_AGG = {s: R.agg_case(*s) for s in [(2, 64), (2, 65), (2, 200), (16, 320), (2, 1000)]}
_CL = {k: R.clamp_case(k) for k in R.CLAMP_KINDS}
_W = {s: R.walk_case(*s) for s in [(3, 127, 3, "nn", 256), (9, 300, 65, "mixed", 256), (3, 300, 200, "random", 256),
                                   (3, 300, 40, "nn", 256), (2, 129, 1024, "mixed", 256), (1, 300, 1024, "random", 1024),
                                   (1, 1, 1, "nn", 256), (9, 1, 200, "nn", 256)]}
_WALKS = [_wk(c) for s, c in _W.items() if s[1] > 1]          # the shapes with more than one point and coarse row
_N1 = [_wk(_W[1, 1, 1, "nn", 256]), _wk(_W[9, 1, 200, "nn", 256])]
# mutation -> the cases built to catch it (a one-point cloud has no short block, no repeated list entry planted, ...)
MUTATIONS = {
    "drop_tile_last": [_agg(_AGG[2, 64]), _agg(_AGG[2, 65]), _agg(_AGG[2, 200]), _agg(_CL["saturated"]), _agg(_CL["scaled"])],
    "drop_cloud_last": [_agg(_AGG[2, 64]), _agg(_AGG[2, 65]), _agg(_AGG[2, 200]), _agg(_CL["zero_cloud"])],
    "drop_chunk": [_agg(_AGG[16, 320]), _agg(_AGG[2, 200]), _agg(_AGG[2, 1000]), _agg(_CL["zero_row"])],
    "cl_shift_swapped": [_agg(_AGG[2, 200]), _agg(_AGG[16, 320]), _agg(_CL["zero_cloud"]), _agg(_CL["saturated"])],
    "flatten_c_major": [_agg(_AGG[2, 200]), _agg(R.selection_case())],
    "no_asum_w2": [_agg(_AGG[2, 200]), _agg(R.selection_case(w2=True)), _agg(_CL["zero_row"]), _agg(_CL["zero_cloud"])],
    "w2_transposed": [_agg(_AGG[2, 200]), _agg(R.selection_case(w2=True))],
    "cluster_not_normalized": [_agg(_AGG[2, 200]), _agg(_AGG[2, 1000]), _agg(_CL["scaled"])],
    "drop_k_mod_256": [_hd(R.head_case(k, 33), 0.0) for k in (120, 136, 264, 1000)],
    "drop_last_8": [_hd(R.head_case(k, 33), 0.0) for k in (8, 136, 264, 1000)] + [_hd(_onehot_head(16384), 0.0)],
    "gate_before_bn1": [_hd(R.head_case(256, 33), 0.0), _hd(R.head_case(1000, 31), 1e-8)],
    "l2_eps_1e12": [_hd(R.head_case(256, 33, clamp=True), 1e-3), _hd(R.head_case(256, 33, gating=False, clamp=True), 1e-3)],
    "walk_wrong_slot": _WALKS,
    "walk_no_rinv": _WALKS + _N1,
    "walk_dup_once": _WALKS + _N1[:1],
    "walk_drop_last": _WALKS + _N1,
    "dist_clamp_1e12": _WALKS,
}


@functools.lru_cache(maxsize=None)
def _effect(name, i):
    """(worst mutated / bound, worst float32 numpy / bound, relative size of the mutation's effect at the element where it
    is detected: |mutated - ref| / max(|mutated|, |ref|) there)"""
    run = MUTATIONS[name][i]
    ref, E = run()
    assert np.isfinite(E).all() and (E >= 0).all()
    mutated = np.asarray(run(mut=(name,))[0], np.float64)
    err = np.abs(mutated - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / E)
    k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[k]), _ratio(run(dt=F32)[0], ref, E), float(err[k] / max(abs(mutated[k]), abs(ref[k])))


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_mutation_is_caught_at_ten_bounds_and_f32_passes(name):
    for i in range(len(MUTATIONS[name])):
        rm, r32, rel = _effect(name, i)
        print("%s case %d: mutated %.3g bounds (relative effect %.3g), float32 numpy %.3g" % (name, i, rm, rel, r32))
        assert rm >= 10.0, "%s case %d: the mutation moves nothing by more than %.3g bounds" % (name, i, rm)
        assert r32 <= 1.0, "%s case %d: float32 numpy is %.3g bounds off" % (name, i, r32)


def test_allowances_sit_ten_times_under_the_smallest_mutation_effect():
    """A_EXP and A_RSQ (relative) against the smallest relative effect any mutation has at the element that detects it."""
    eff = {(n, i): _effect(n, i)[2] for n in MUTATIONS for i in range(len(MUTATIONS[n]))}
    k = min(eff, key=eff.get)
    print("smallest relative mutation effect %.3g (%s case %d); A_EXP %.3g A_RSQ %.3g" % (eff[k], k[0], k[1], R.A_EXP, R.A_RSQ))
    assert 10 * max(R.A_EXP, R.A_RSQ) <= eff[k]


@pytest.mark.parametrize("shape", R.AGG_SHAPES)
def test_float32_aggregate_is_under_the_bound(shape):
    case = R.agg_case(*shape)
    for gating in (True, False):
        hp = R.head_params(R.seed("f32", shape, gating), R.DM * R.CL, gating)
        ref, E = R.fused(*case, *hp, 1e-8)
        assert _ratio(R.fused(*case, *hp, 1e-8, dt=F32)[0], ref, E) <= 1.0
    ref, E = R.aggregate(*case)
    assert _ratio(R.aggregate(*case, dt=F32)[0], ref, E) <= 1.0


@pytest.mark.parametrize("shape", R.WALK_SHAPES)
def test_float32_walk_is_under_the_bound(shape):
    case = R.walk_case(*shape)
    ref, g = R.walk_ref(case), R.walk_ref(case, dt=F32)
    for k, what in ((0, "att"), (2, "apart"), (4, "asum")):
        assert _ratio(g[k], ref[k], ref[k + 1]) <= 1.0, what


@pytest.mark.parametrize("m", R.TAIL_M)
def test_float32_tail_is_under_the_bound(m):
    case = R.tail_case(9, m)
    ref, E = R.tail_assign(*case, 1e-8)
    assert _ratio(R.tail_assign(*case, 1e-8, dt=F32)[0], ref, E) <= 1.0


@pytest.mark.parametrize("kind", R.CLAMP_KINDS)
def test_float32_clamp_cases_are_finite_and_under_the_bound(kind):
    case = R.clamp_case(kind)
    hp = R.head_params(R.seed("clamp", kind), R.DM * R.CL)
    for fn, args in ((R.aggregate, case), (R.fused, case + hp + (1e-8,))):
        ref, E = fn(*args)
        got = fn(*args, dt=F32)[0]
        assert np.isfinite(ref).all() and np.isfinite(E).all() and np.isfinite(got).all()
        assert _ratio(got, ref, E) <= 1.0
    ref, E = R.aggregate(*case)                    # the bound stays a bound, not a licence: a tenth of a unit vector's
    big = np.abs(ref) > 1e-3                       # larger entries at the most
    assert big.any() and (E[big] <= 0.1 * np.abs(ref[big])).all()


# ------------------------------------------------------------------------------------------------------- degenerate
def test_zero_attention_cloud_gives_zero_vlad_and_the_bn1_shift():
    x, att, Wc, sc, sh, W2 = R.agg_case(2, 65)
    att[1] = 0
    vl, E, f = R.aggregate(x, att, Wc, sc, sh, W2, detail=True)
    assert not vl[1].any() and E[1].max() < 1e-20 and vl[0].any()     # (the bound: the underflow floor alone)
    hp = R.head_params(R.seed("deg"), R.DM * R.CL, gating=False)
    out, _ = R.fused(x, att, Wc, sc, sh, W2, *hp, 0.0)
    assert np.array_equal(out[1], hp[2].astype(np.float64))


def test_zero_row_adds_att_softmax_of_the_shift_to_asum_and_nothing_to_v():
    x, att, Wc, sc, sh, W2 = R.agg_case(2, 65)
    _, _, f0 = R.aggregate(np.delete(x, 7, 1), np.delete(att, 7, 1), Wc, sc, sh, W2 * 0, detail=True)
    x[:, 7] = 0
    _, _, f1 = R.aggregate(x, att, Wc, sc, sh, W2 * 0, detail=True)
    e = np.exp(sh.astype(np.float64) - sh.max())
    assert np.abs(f1["asum"] - f0["asum"] - att[:, 7, None] * e / e.sum()).max() < 1e-15
    assert np.abs(f1["v"] - f0["v"]).max() < 1e-15
