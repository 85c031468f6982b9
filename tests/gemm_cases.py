"""Cases, operand builders and expected values of tests/test_gemm_kernels_gpu.py: the training GEMMs of csrc/gemm.hip
(dh3d_gemm_tn_f32, dh3d_gemm_nn_f32, their batched forms) kernel by kernel.  No GPU and no torch here;
tests/test_gemm_cases.py pins this module, the dispatch of every case included.

A case is FILED under the kernel it was written for (`kernel`, a name of pm.GEMM_KERNELS) and under the state of its
reduction (`split`: more than one chunk, the partials then meet in atomics; `chunks` / `last`: the chunk count and the
length of the last chunk where the case exists for exactly that).  `filed_ok` compares that with dh3d_gemm_plan.

Shapes are (M, K, N) throughout, M x N the output and K the reduction, whatever the form: the tn form stores the
row operand as [K, M].  Builders return the LOGICAL operands X [batch, M, K] and Y [batch, K, N]; `device_operands` lays
X out for the form.

Probes (every expected value exact, or a single product):
  integers       : entries in [-8, 8]; K * 64 (+ |C0|) < 2^24, so every partial sum is an integer below 2^24 and exact
                   in f32 in any order -- across split chunks and atomics too.  Lives in the first bf16 chunk only.
  three_chunks   : one operand dense with integers of 20 significant bits (all three bf16 chunks in use), the other with at
                   most 8 entries of +-1 per output line: sums below 2^23, exact.  Needs c1 d1, c2 d1, c3 d1 (X dense) or
                   c1 d1, c1 d2, c1 d3 (Y dense).
  second_order   : 1 + 2^-9 against 1 + 2^-9, one nonzero per line: 1 + 2^-8 + 2^-18 exactly, and only with c2 d2.
  single_product : one nonzero per line, full-mantissa values: within SINGLE_PRODUCT_BOUND of the float64 product.
  dense          : full-mantissa or wide-magnitude operands against bound(T, K) = (K + 16) 2^-24 T."""
import collections

import numpy as np

from dense_reference import SINGLE_PRODUCT_BOUND, SIX, bound, six_products, split3  # noqa: F401  (re-exported)

F64 = np.float64
KERNEL_ORDER = ((3, 1), (1, 3), (2, 2), (2, 1), (1, 2), (1, 1))   # gemm_x6_kernel: small terms first
V9 = np.float32(1 + 2.0 ** -9)
V9_SQUARED = np.float32(1 + 2.0 ** -8 + 2.0 ** -18)

Case = collections.namedtuple("Case", "form M K N kernel split batch bias chunks last")


def case(form, M, K, N, kernel, split, batch=1, bias=False, chunks=None, last=None):
    assert form in ("nn", "tn") and not (bias and form == "tn")
    return Case(form, M, K, N, kernel, bool(split), batch, bool(bias), chunks, last)


def case_id(c):
    return "%s-%s%dx%dx%d%s-%s" % (c.kernel, "%dx" % c.batch if c.batch > 1 else "", c.M, c.K, c.N,
                                   "+bias" if c.bias else "", c.form)


# ------------------------------------------------------------------------------------------------------ the case table
def _rows_cases():
    """gemm_rows_kernel<RB> (nn, M <= 32, K <= 512): every RB step, the per-wave K quarter at K % 64 != 0, N around 64 and
    128.  Every (M, K) pair, N cycling."""
    Ms, Ks, Ns = (1, 8, 9, 16, 17, 24, 25, 32), (4, 60, 64, 68, 252, 256, 512), (4, 60, 64, 68, 132)
    out = []
    for i, M in enumerate(Ms):
        for j, K in enumerate(Ks):
            out.append(case("nn", M, K, Ns[(i + j) % len(Ns)], "rows%d" % ((M + 7) // 8), False))
    out.append(case("nn", 32, 512, 132, "rows4", False))
    out.append(case("nn", 1, 4, 4, "rows1", False))
    return out


def _shortk_cases():
    """gemm_shortk_kernel (tn, K <= 32): the whole cube of the edges."""
    edge = (4, 60, 64, 68, 132)
    return [case("tn", M, K, N, "shortk", False) for K in (1, 2, 31, 32) for M in edge for N in edge]


def _f32_cases():
    """gemm_f32_kernel<TA, 2, WN>: M around 128 and 256, N around 64 (narrow) and 128 / 256 (wide), K off the 16-step
    stage, the last, shorter chunk.  Every (M, N) pair, K cycling.  The reduction is split exactly when K exceeds one
    minimum chunk (64 steps of tn, 256 of nn): few tiles, so the workgroup target never binds before that."""
    Ms, narrow, wide = (4, 124, 128, 132, 260), (4, 60, 64), (68, 128, 132, 260)
    tnK, nnK = (33, 47, 48, 49, 70, 1000, 1001), (20, 36, 52, 1000, 4000)
    out = []
    for form, Ks, kmin in (("tn", tnK, 64), ("nn", nnK, 256)):
        for i, M in enumerate(Ms):
            for j, N in enumerate(narrow + wide):
                ks = Ks if (form == "tn" or M > 32) else tuple(k for k in Ks if k > 512)   # (nn, M <= 32, K <= 512: rows)
                ks = tuple(k for k in ks if k % 32 or float(M) * N * k < 2.0 ** 26)        # (260 x 4000 x 132: bf16x6)
                K = ks[(i + j) % len(ks)]
                out.append(case(form, M, K, N, "f32_narrow" if N <= 64 else "f32_wide", K > kmin))
    out += [
        case("tn", 132, 70, 68, "f32_wide", True, chunks=2, last=22),
        case("nn", 129, 1000, 132, "f32_wide", True, chunks=4, last=232),
        # where a product leaves the plain-FMA kernels: M 32 -> 33, K 512 -> 516 (nn), K 32 -> 33 (tn)
        case("nn", 33, 36, 68, "f32_wide", False), case("nn", 32, 516, 68, "f32_wide", True),
        case("tn", 68, 33, 60, "f32_narrow", False),
        # just under the bf16x6 threshold: K % 32 != 0 on either side of K = 2048
        case("nn", 256, 2016, 128, "f32_wide", True), case("nn", 256, 2064, 128, "f32_wide", True),
        # N = 60 keeps these under 2^26 multiply-adds
        case("nn", 512, 2048, 60, "f32_narrow", True), case("tn", 128, 8192, 60, "f32_narrow", True),
        # batched: a batch of tiny products runs on the tiles, not on the plain-FMA kernels
        case("nn", 130, 36, 20, "f32_narrow", False, batch=3, bias=True), case("nn", 8, 64, 68, "f32_wide", False, batch=3),
        case("nn", 130, 1000, 132, "f32_wide", True, batch=3), case("tn", 36, 70, 132, "f32_wide", True, batch=3),
        case("tn", 64, 16, 60, "f32_narrow", False, batch=5),
        case("nn", 124, 36, 64, "f32_narrow", False, bias=True), case("nn", 260, 1000, 260, "f32_wide", False, bias=True,
                                                                      chunks=1),
    ]
    return out


X6_CASES = [
    case("nn", 256, 2048, 128, "x6_wide", True, chunks=8),
    case("nn", 1024, 256, 256, "x6_wide", False, chunks=1),                  # interior store, no atomics
    case("nn", 129, 4096, 132, "x6_wide", True),                              # ragged in M and N
    case("nn", 260, 2080, 132, "x6_wide", True, chunks=9, last=32),           # ragged last chunk
    case("nn", 512, 2048, 64, "x6_narrow", True),
    case("nn", 580, 2048, 60, "x6_narrow", True),                             # ragged; 580 rows reach 2^26 at N = 60
    case("tn", 256, 2048, 128, "x6_wide", True, chunks=32),
    case("tn", 132, 4128, 132, "x6_wide", True, chunks=65, last=32),
    case("tn", 128, 8192, 64, "x6_narrow", True),
    case("tn", 140, 8192, 60, "x6_narrow", True),                             # ragged; 140 columns of A reach 2^26
    case("nn", 256, 2048, 128, "x6_wide", False, bias=True, chunks=1),        # a bias forces one chunk
    case("nn", 130, 512, 68, "x6_wide", True, batch=16),
    case("tn", 64, 1024, 132, "x6_wide", True, batch=8),
]

FAMILIES = collections.OrderedDict([("rows", _rows_cases()), ("shortk", _shortk_cases()), ("f32", _f32_cases()),
                                    ("x6", X6_CASES)])

# the four bf16x6 instantiations at a ragged shape each, and a batched one: the probes of (a') (b) (c)
X6_PROBE_CASES = [X6_CASES[3], X6_CASES[5], X6_CASES[7], X6_CASES[9], X6_CASES[11]]

# (d): one edge shape per kernel instantiation
DENSE_CASES = [
    case("nn", 7, 252, 68, "rows1", False), case("nn", 9, 60, 132, "rows2", False), case("nn", 17, 512, 60, "rows3", False),
    case("nn", 25, 68, 4, "rows4", False), case("nn", 32, 256, 64, "rows4", False, bias=True),
    case("tn", 68, 31, 132, "shortk", False), case("tn", 132, 1, 60, "shortk", False),
    case("tn", 132, 1001, 60, "f32_narrow", True), case("tn", 260, 49, 132, "f32_wide", False),
    case("nn", 129, 1000, 60, "f32_narrow", True), case("nn", 133, 52, 68, "f32_wide", False, bias=True),
    case("nn", 130, 36, 20, "f32_narrow", False, batch=3, bias=True), case("tn", 36, 70, 132, "f32_wide", True, batch=3),
] + X6_PROBE_CASES + [X6_CASES[10], X6_CASES[12]]


def instantiation(c):
    """the template instantiation a case runs: the kernel with its form where the form is a template argument"""
    return c.kernel if c.kernel.startswith(("rows", "shortk")) else "%s_%s" % (c.kernel, c.form)


def filed_ok(c, plan, is_split):
    """plan = pm.gemm_plan(...) = (kernel, chunks, kchunk, stage) or None, is_split = dh3d_gemm_is_split(...) -> None, or
    what moved."""
    if plan is None:
        return "refused"
    kernel, chunks, kchunk, stage = plan
    last = c.K - (chunks - 1) * kchunk
    if kernel != c.kernel:
        return "kernel %s" % kernel
    if (chunks > 1) != c.split or (c.chunks is not None and chunks != c.chunks) or (c.last is not None and last != c.last):
        return "%d chunks of %d, the last %d" % (chunks, kchunk, last)
    if chunks > 1 and not is_split:
        return "split, but dh3d_gemm_is_split says 0"
    return None


# ------------------------------------------------------------------------------------------------------------ operands
def rng_of(c, salt=0):
    return np.random.default_rng([c.M, c.K, c.N, c.batch, int(c.form == "tn"), int(c.bias), salt])


def full_mantissa(rng, shape):
    """mixed sign, magnitude 2^-6 .. 2^6, all 24 significand bits in use (the lowest one set)."""
    mant = rng.integers(0, 1 << 22, shape).astype(np.uint32) << np.uint32(1) | np.uint32(1)
    expo = rng.integers(127 - 6, 127 + 6, shape).astype(np.uint32) << np.uint32(23)
    sign = rng.integers(0, 2, shape).astype(np.uint32) << np.uint32(31)
    return (sign | expo | mant).view(np.float32)


def wide(rng, shape):
    return (rng.standard_normal(shape) * np.exp(rng.uniform(-8, 8, shape))).astype(np.float32)


def device_operands(c, X, Y):
    """(A, B) as the entry point of the case's form stores them: nn A = X [.., M, K]; tn A = X^T [.., K, M]."""
    A = X if c.form == "nn" else np.ascontiguousarray(np.swapaxes(X, -1, -2))
    return np.ascontiguousarray(A), np.ascontiguousarray(Y)


def integer_operands(c, rng):
    """X, Y in [-8, 8], C0 in [-1000, 1000], bias in [-100, 100] (all f32 holding integers) and the exact products
    want [batch, M, N] as int64.  Every batch entry differs."""
    assert c.K * 64 + 1000 < 2 ** 24
    X = rng.integers(-8, 9, (c.batch, c.M, c.K)).astype(np.float32)
    Y = rng.integers(-8, 9, (c.batch, c.K, c.N)).astype(np.float32)
    C0 = rng.integers(-1000, 1001, (c.batch, c.M, c.N)).astype(np.float32)
    bias = rng.integers(-100, 101, (c.batch, c.N)).astype(np.float32)
    want = np.rint(X.astype(F64) @ Y.astype(F64)).astype(np.int64)      # integers below 2^24: exact in float64
    assert np.abs(want).max() + 1000 < 2 ** 24
    return X, Y, C0, bias, want


def probe_positions(K, kchunk, count):
    """`count` reduction indices that visit, first, both sides of every chunk boundary, then every residue mod 32 (both
    halves of a 16- or 32-step stage) in a chunk that moves with the residue, then a stride that is odd against both."""
    chunks = -(-K // kchunk)
    ks = []
    for b in range(1, chunks):
        ks += [b * kchunk - 1, b * kchunk]
    ks += [((r * 7) % chunks * kchunk + r) % K for r in range(32)]
    ks += [0, K - 1]
    i = 0
    while len(ks) < count:
        ks.append((i * (kchunk + 33) + 5) % K)
        i += 1
    return np.asarray(ks[:max(count, 0)], np.int64), len(ks) <= count


def positions_cover(ks, K, kchunk):
    """do these indices hit every residue mod 32, and the first and the last index of every chunk that has a neighbour?"""
    chunks = -(-K // kchunk)
    s = set(int(k) for k in np.ravel(ks))
    sides = all((b * kchunk - 1) in s and (b * kchunk) in s for b in range(1, chunks))
    return sides and set(k % 32 for k in s) == set(range(32))


def _dense20(rng, shape):
    """integers of 20 significant bits, mixed sign: bits 19, 10 and 0 set, so c1, c2 and c3 are all nonzero."""
    v = rng.integers(0, 1 << 19, shape) | (1 << 19) | (1 << 10) | 1
    return (v * rng.choice([-1, 1], shape)).astype(np.float32)


def three_chunk_operands(c, kchunk, rng, dense):
    """dense = 'X': X dense 20-bit integers, Y at most 8 entries of +-1 per column; dense = 'Y': the mirror (at most 8 per
    row of X).  -> X, Y, want int64, and whether the sparse operand's positions cover what probe_positions promises."""
    lines = c.N if dense == "X" else c.M
    ks, fits = probe_positions(c.K, kchunk, 8 * lines)
    assert fits, "too few lines for the chunk boundaries of this case"
    ks = ks.reshape(lines, 8)
    X = np.zeros((c.batch, c.M, c.K), np.float32)
    Y = np.zeros((c.batch, c.K, c.N), np.float32)
    for b in range(c.batch):
        sign = rng.choice(np.float32([-1, 1]), (lines, 8))
        rot = np.roll(ks, b, axis=0)                                  # every batch entry its own positions
        if dense == "X":
            X[b] = _dense20(rng, (c.M, c.K))
            for t in range(8):
                Y[b, rot[:, t], np.arange(lines)] = sign[:, t]
        else:
            Y[b] = _dense20(rng, (c.K, c.N))
            for t in range(8):
                X[b, np.arange(lines), rot[:, t]] = sign[:, t]
    sparse = Y if dense == "X" else np.swapaxes(X, 1, 2)
    assert (sparse != 0).sum(1).max() <= 8
    assert all((ch != 0).all() for ch in split3(X if dense == "X" else Y)), "a dense entry leaves a chunk empty"
    want = np.rint(X.astype(F64) @ Y.astype(F64)).astype(np.int64)
    assert np.abs(want).max() < 2 ** 23
    return X, Y, want, positions_cover(ks, c.K, kchunk)


def line_positions(c, kchunk, lines, shift=0):
    """one reduction index per line: the chunk and the residue mod 32 both advance by one from line to line, and the
    32-step block inside the chunk every 32 lines (kchunk and the last chunk are multiples of 32 on the bf16x6 kernel), so
    `lines` >= max(32, chunks) visit every residue and every chunk."""
    assert kchunk % 32 == 0 and c.K % 32 == 0
    m = np.arange(lines, dtype=np.int64) + shift
    chunk = m % (-(-c.K // kchunk))
    clen = np.minimum(kchunk, c.K - chunk * kchunk)
    return chunk * kchunk + (m % 32 + 32 * (m // 32)) % clen


def lines_cover(ks, K, kchunk):
    chunks = -(-K // kchunk)
    return set(int(k) % 32 for k in ks) == set(range(32)) and set(int(k) // kchunk for k in ks) == set(range(chunks))


def second_order_operands(c, kchunk, sparse="X"):
    """sparse = 'X': one V9 per row of X, Y all V9; 'Y': one V9 per column of Y, X all V9.  Every output element is
    V9_SQUARED exactly.  -> X, Y, covered."""
    X = np.full((c.batch, c.M, c.K), V9 if sparse == "Y" else 0, np.float32)
    Y = np.full((c.batch, c.K, c.N), V9 if sparse == "X" else 0, np.float32)
    lines = c.M if sparse == "X" else c.N
    cover = True
    for b in range(c.batch):
        ks = line_positions(c, kchunk, lines, shift=3 * b)
        cover = cover and lines_cover(ks, c.K, kchunk)
        if sparse == "X":
            X[b, np.arange(lines), ks] = V9
        else:
            Y[b, ks, np.arange(lines)] = V9
    return X, Y, cover


def single_product_operands(c, kchunk, rng):
    """one full-mantissa nonzero a[b, m] per row of X at k(b, m), Y full-mantissa -> X, Y, a [batch, M], rows
    Y[b, k(b, m), :] [batch, M, N], covered.  The float64 product a * rows is the expected value."""
    X = np.zeros((c.batch, c.M, c.K), np.float32)
    Y = full_mantissa(rng, (c.batch, c.K, c.N))
    a = full_mantissa(rng, (c.batch, c.M))
    rows = np.empty((c.batch, c.M, c.N), np.float32)
    cover = True
    for b in range(c.batch):
        ks = line_positions(c, kchunk, c.M, shift=5 * b)
        cover = cover and lines_cover(ks, c.K, kchunk)
        X[b, np.arange(c.M), ks] = a[b]
        rows[b] = Y[b, ks]
    return X, Y, a, rows, cover


def dense_reference(X, Y, C0=None, bias=None):
    """float64 value and first-order error scale T of X @ Y (+ C0) (+ bias[:, None, :])."""
    X64, Y64 = X.astype(F64), Y.astype(F64)
    v, T = X64 @ Y64, np.abs(X64) @ np.abs(Y64)
    if C0 is not None:
        v, T = v + C0, T + np.abs(C0.astype(F64))
    if bias is not None:
        v, T = v + bias[:, None, :], T + np.abs(bias.astype(F64))[:, None, :]
    return v, T


def emulate_x6(X, Y, keep=KERNEL_ORDER):
    """A restatement of gemm_x6_kernel for ONE batch entry: the chunk products of `keep` (exact in f32), summed in float64."""
    c, d = split3(X), split3(Y)
    out = np.zeros((X.shape[0], Y.shape[1]), F64)
    for i, j in keep:
        out += c[i - 1].astype(F64) @ d[j - 1].astype(F64)
    return out
