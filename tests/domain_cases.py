"""Seeded RadianceQuery rows over the whole query domain (helper module of the domain tests, not a test).

``synthetic.cornell_queries`` keeps positions in [-0.05, 0.05]^3, roughness at 1 and specular at 0 for 90 % of its rows.
The rows here cover what a renderer can hand over:

(a) ``bulk_rows``     positions U[0, 1)^3 with a 20 % share in [-0.2, 1.2]^3, theta U[0, pi], phi U(-pi, pi],
                      roughness / diffuse / specular U[0, 1];
(b) ``branch_rows``   every value at which an encoder takes another path (list below), one special value in a row of
                      otherwise bulk values, so that a failing row names one feature, plus a few rows that combine
                      specials of every field class;
(c) ``hostile_rows``  NaN, +-inf and 1e30 in each field class: only for the tests that such a row changes nothing but
                      its own output. Never compared with an oracle.

``domain_queries`` is (a) + (b) shuffled; every function is deterministic from its seed and returns (n, 15) float32.
Padded callers insert pad_ themselves (``padded``).
"""
import numpy as np

SEED = 20251126
POS, BLOB, IDENT = slice(0, 3), slice(3, 9), slice(9, 15)  # TriangleWave / HashGrid, OneBlob and Identity inputs
HASH_POS_MAX = 1024.0  # Hash: floorf(scale * p + 0.5) fits an int32 up to here (scale <= 16 * 2^15 - 1)
HASH_LEVELS = (0, 1, 5, 15)


def _f32(x):
    return np.asarray(x, np.float32)


def _around(v):
    """v and its two float32 neighbours"""
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


def bulk_rows(n, seed=SEED):
    rng = np.random.default_rng([seed, 1])
    q = np.empty((n, 15), np.float32)
    pos = rng.random((n, 3))
    wide = rng.random(n) < 0.2
    pos[wide] = rng.uniform(-0.2, 1.2, (int(wide.sum()), 3))
    q[:, POS] = pos
    for c in (3, 5):  # direction, normal: (theta, phi)
        q[:, c] = rng.uniform(0.0, np.pi, n)
        q[:, c + 1] = -rng.uniform(-np.pi, np.pi, n)  # (-pi, pi]
    q[:, 7:15] = rng.random((n, 8))
    q[:, POS] = np.minimum(q[:, POS], np.where(wide[:, None], np.float32(1.2), np.nextafter(np.float32(1), np.float32(0))))
    return q


def position_specials(hash_safe=False):
    tiny = np.float32(2.0 ** -149)
    v = [0.0, -0.0, tiny, -tiny, 1e-9, -1e-9, 0.5]
    v += _around(1.0) + [_around(0.25)[0], _around(0.25)[2]]
    for k in (1, 2, 1023, 2047, 2048, 2049, 3071, 4095):  # kinks of the top octave (2^11 x): tri = 0 or 1 there
        a = _around(k / 4096.0)
        v += [a[0], a[2]]
    for l in HASH_LEVELS:
        s = 16 * 2 ** l - 1
        v += [np.float32(k / s) for k in (1, 2, s // 2, s - 1)]  # cell boundaries: fraction 0
        v += [np.float32(-1.0 / s)]                              # cell -1
    v += [3.7, -3.7, 100.25, HASH_POS_MAX]
    if not hash_safe:
        v += [2.0 ** 20 + 0.5]
    return _f32(v)


def blob_specials():
    v = []
    for k in range(-6, 10):  # multiples of 1/4 in [-1.5, 2.25]: t = 4x = -6 .. 9 with fr = 0, the wrap clamps included
        v += _around(k / 4.0)
    return _f32(v + [np.pi, -np.pi, 64.0, -64.0])


def ident_specials():
    return _f32([0.0, -0.0, 65504.0, 65520.0, 1e-8])  # 65520 rounds to f16 inf


def branch_rows(seed=SEED, hash_safe=False):
    """One row per (special value, field of its class), otherwise bulk values; then 24 rows that draw every field
    from its class's specials."""
    ps, bs, is_ = position_specials(hash_safe), blob_specials(), ident_specials()
    single = [(c, v) for v in ps for c in range(0, 3)] + [(c, v) for v in bs for c in range(3, 9)] + \
             [(c, v) for v in is_ for c in range(9, 15)]
    q = bulk_rows(len(single) + 24, seed + 1)
    for r, (c, v) in enumerate(single):
        q[r, c] = v
    rng = np.random.default_rng([seed, 2])
    tame_p = ps[np.abs(ps) <= 4.0]
    tame_i = is_[np.abs(is_) < 65504.0]  # the f16-overflow values have rows of their own (f16_overflow_rows)
    for r in range(len(single), len(q)):
        q[r, POS] = rng.choice(tame_p, 3)
        q[r, BLOB] = rng.choice(bs, 6)
        q[r, IDENT] = rng.choice(tame_i, 6)
    return q


def domain_queries(n, seed=SEED, hash_safe=False):
    """n rows of (a) + (b): every branch row and bulk rows for the rest, in a seeded order."""
    b = branch_rows(seed, hash_safe)
    assert n >= len(b), f"the branch rows alone are {len(b)}"
    q = np.concatenate([b, bulk_rows(n - len(b), seed)])
    return np.ascontiguousarray(q[np.random.default_rng([seed, 3]).permutation(n)])


def f16_overflow_rows(q):
    """Rows with an Identity input at the end of the f16 range: 65520 rounds to f16 inf, and 65504 (the largest f16)
    times a layer-0 weight of the parity tests' networks (|w| up to 0.27) gives hidden activations of 1e4 whose
    layer-1 sums pass 65504, so the f16 activations of the oracle itself (MIXED, TCNN) overflow there too
    (test_domain_oracle.py asserts that no other row does). The network output of these rows is inf / NaN by the
    numerics model, so they take part in the encoder comparisons only."""
    return (np.abs(_f32(q)[:, -6:]) >= np.float32(65504.0)).any(axis=1)


def hash_unsafe_rows(q):
    return (np.abs(_f32(q)[:, :3]) > HASH_POS_MAX).any(axis=1)


def network_rows(q, hash_safe=False):
    """The rows of q that the network-level comparisons use"""
    keep = ~f16_overflow_rows(q)
    if hash_safe:
        keep &= ~hash_unsafe_rows(q)
    return np.ascontiguousarray(_f32(q)[keep])


def hostile_rows(seed=SEED):
    """(c): one non-finite or huge value in one field class per row, then whole classes and the whole row"""
    bad = [np.nan, np.inf, -np.inf]
    cases = [(cls, v) for cls in (POS, BLOB, IDENT) for v in bad] + [(POS, 1e30), (POS, -1e30), (BLOB, 1e30), (BLOB, -1e30)]
    q = bulk_rows(2 * len(cases) + 2, seed + 2)
    rng = np.random.default_rng([seed, 4])
    for r, (cls, v) in enumerate(cases):
        q[r, rng.integers(cls.start, cls.stop)] = v  # one field
        q[len(cases) + r, cls] = v                   # the whole class
    q[-2] = np.nan
    q[-1, POS], q[-1, BLOB], q[-1, IDENT] = np.inf, -np.inf, np.nan
    return q


def padded(q15, pad):
    """(n, 15) compact records -> (n, 16) padded records with pad_ = pad (scalar or (n,))"""
    q = _f32(q15)
    return np.ascontiguousarray(np.insert(q, 3, np.broadcast_to(_f32(pad), (q.shape[0],)), axis=1), np.float32)


def pad_values(n, seed=SEED):
    return np.random.default_rng([seed, 5]).uniform(-1.0, 1.0, n).astype(np.float32)


# ---- parameter blocks of the gradient comparisons -------------------------------------------------------------------
def mlp_blocks(width=64, inw=80, layout="frequency"):
    """name -> flat index array into the canonical blob W0[width][inw], W1..W4[width][width], W5[16][width]; layer 0
    split by the feature class of its columns. layout: frequency | padded | sh | hash | hash_padded (the column order
    of each encoding, include/nrc/layout.h)."""
    cols = {"frequency": {"tri": (0, 36), "oneblob": (36, 60), "identity": (60, 66), "pad": (66, 80)},
            "padded": {"tri": (0, 36), "pad_": (36, 37), "oneblob": (37, 61), "identity": (61, 67), "pad": (67, 80)},
            "sh": {"tri": (0, 36), "sh": (36, 52), "oneblob": (52, 68), "identity": (68, 74), "pad": (74, 80)},
            "hash": {"grid": (0, 32), "oneblob": (32, 56), "identity": (56, 62), "pad": (62, 64)},
            "hash_padded": {"grid": (0, 32), "pad_": (32, 33), "oneblob": (33, 57), "identity": (57, 63),
                            "pad": (63, 64)}}[layout]
    blocks, w0 = {}, np.arange(width * inw).reshape(width, inw)
    for name, (lo, hi) in cols.items():
        blocks[f"W0.{name}"] = w0[:, lo:hi].ravel()
    off = width * inw
    for l in range(1, 5):
        blocks[f"W{l}"] = np.arange(off, off + width * width)
        off += width * width
    blocks["W5"] = np.arange(off, off + 16 * width)
    return blocks


def hash_level_blocks(mlp_params=21504):
    """name -> slice of the Hash blob holding level l's table ([entry][2]; level 0: 4096 entries, others 32768)"""
    out, e = {}, 0
    for l in range(16):
        cnt = 4096 if l == 0 else 32768
        out[f"grid.L{l}"] = slice(mlp_params + 2 * e, mlp_params + 2 * (e + cnt))
        e += cnt
    return out


# ---- the network-level cases shared by the CPU fitness test and the GPU tests ---------------------------------------
# Row count of the inference parity tests: every branch row and bulk rows for the rest. The existing per-row rule (at
# most 0.1 % of the rows beyond 16 f16 ulps) must not be spent by the oracle's own sensitivity: the three rows with a
# position of 2^20 + 0.5 (one ulp there is 1/16, a whole period of octave 4) always move that far under a one-ulp nudge,
# and half the cap has to hold them with room for the bulk: 0.0005 n = 8. 16,385 is also a ragged last tile after 512
# full ones. The training batches (train_queries) put the branch rows first.
N_INFER = 16385
GRAD_CASES = [("frequency", 100), ("frequency", 1000), ("frequency", 4608), ("padded", 1000), ("sh", 1000),
              ("wide", 1000), ("hash", 1000)]
_POOL = {}


def domain_pool(hash_safe=False):
    """The domain rows whose network rows are exactly N_INFER: N_INFER + the number of f16-overflow branch rows"""
    extra = int(f16_overflow_rows(branch_rows(SEED, hash_safe)).sum())
    return domain_queries(N_INFER + extra, SEED, hash_safe)


def pool(hash_safe=False):
    """The N_INFER network rows (no Identity input at the end of the f16 range; Hash: |p| <= 1024), computed once"""
    if hash_safe not in _POOL:
        _POOL[hash_safe] = network_rows(domain_pool(hash_safe), hash_safe)
        assert len(_POOL[hash_safe]) == N_INFER
        _POOL[hash_safe].setflags(write=False)
    return _POOL[hash_safe]


def damp_octaves(params, width=64):
    """Layer 0's triangle-wave column of octave k scaled by 2^-k. The wave of octave k has slope 2^(k+1), so a position
    step of one f32 ulp moves the top octave's feature 2^11 times as far as octave 0's; with weights of one magnitude
    in every octave (any random draw) the oracle itself moves 0.2 % - 0.9 % of the domain rows by more than the parity
    tests' 16 output ulps under that step (measured on ORC_MIXED alone with the golden, the init and the xavier
    weights), more than the 0.1 % those tests allow the kernel. Scaled so, every octave answers a position step alike,
    as a network fitted to a band-limited radiance field does, and the oracle moves 3 - 7 of 16,385 rows. A wrong
    feature of the top octave (error O(1) x weight 0.3 x 2^-11 = 1.5e-4 of a pre-activation) is left to the encoder
    tests, which compare every feature; these weights are for the network-level comparisons."""
    p = np.array(params, np.float32)
    p[:width * 80].reshape(width, 80)[:, :36] *= np.tile(np.float32(2.0) ** -np.arange(12, dtype=np.float32), 3)
    return p


def case_queries(kind, n):
    """The first n network rows in the record layout of the case (padded: random pad_ values)"""
    q = pool(kind.startswith("hash"))[:n]
    assert len(q) == n
    return padded(q, pad_values(n)) if kind.endswith("padded") else q.copy()


def train_queries(kind, b):
    """A training batch of b rows: every network-usable branch row (about 500; b = 100: a fixed sample of 80 of them),
    bulk rows for the rest, in a seeded order so that the branch rows spread over the kernels' sample blocks"""
    h = kind.startswith("hash")
    br = network_rows(branch_rows(SEED, h), h)
    if b < len(br):
        br = br[np.sort(np.random.default_rng([SEED, 6, b]).choice(len(br), (4 * b) // 5, replace=False))]
    q = np.concatenate([br, bulk_rows(b - len(br), SEED + 3)])
    q = np.ascontiguousarray(q[np.random.default_rng([SEED, 7, b]).permutation(b)])
    return padded(q, pad_values(b)) if kind.endswith("padded") else q


def train_targets(nrc, b):
    return nrc.synthetic.cornell_targets(b, seed=300 + b)


def case_params(kind, orc, golden):
    """The weights of each path's existing parity test, with the spatial encoding's weights scaled per octave / level
    so that the oracle alone stays inside the parity tests' outlier cap on this domain (damp_octaves)"""
    if kind.startswith("hash"):
        from test_gpu_hash import _trained_like
        p = _trained_like(orc)
        # level l's table scaled by 2^(-3l/4): a position step of one f32 ulp is 16 x 2^l ulps of a cell at level l, so a
        # table of one amplitude at every level makes half the rows move by more than the parity tests' 16 output ulps
        # under that step (measured on the oracle alone: 2,007 of 4,097 rows). The full 2^-l of damp_octaves would put
        # the finest level (3e-5) among the f16 subnormals; at 2^(-3l/4) it keeps 4e-4, a normal f16 of ulp 2.4e-7,
        # so a wrong entry there is still two hundred times the encoder test's 2e-6
        for name, sl in hash_level_blocks(orc.HASH_MLP_PARAMS).items():
            p[sl] *= np.float32(2.0 ** (-0.75 * int(name[6:])))
        return p
    if kind.startswith("wide"):
        from test_gpu_wide import wide_params
        return damp_octaves(wide_params(21, gain=1.2), 128)
    return damp_octaves(golden["params_b"])


def case_blocks(kind):
    if kind == "hash":
        return {**mlp_blocks(64, 64, "hash"), **hash_level_blocks()}
    if kind == "wide":
        return mlp_blocks(128, 80, "frequency")
    return mlp_blocks(64, 80, kind)


def oracle_forward(orc, kind, params, q, mode):
    if kind == "hash":
        return orc.hash_forward(params, q, mode)
    if kind == "hash_padded":
        return orc.hash_forward(params, q, mode, padded=True)
    if kind == "wide":
        return orc.wide_forward(params, q, mode)
    enc = {"frequency": orc.FREQUENCY, "sh": orc.FREQUENCY_SH, "padded": orc.FREQUENCY | orc.PADDED}[kind]
    return orc.forward(params, q, mode, encoding=enc)


def oracle_grad(orc, kind, params, q, t, mode, n_total=None):
    """(loss-scaled gradient in the API's column order, loss); n_total: 3 x the global batch when q is a part of it"""
    if kind == "hash":
        return orc.hash_grad(params, q, t, n_total=n_total, mode=mode)
    if kind == "wide":
        return orc.wide_grad(params, q, t, n_total=n_total, mode=mode)
    enc = {"frequency": orc.FREQUENCY, "sh": orc.FREQUENCY_SH, "padded": orc.FREQUENCY | orc.PADDED}[kind]
    return orc.grad(params, q, t, n_total=n_total, mode=mode, encoding=enc)


def kink_rows(orc, kind, params, q, eps=2e-3):
    """Rows with an output channel at the output ReLU's kink: 0 < y <= eps in ORC_MIXED or ORC_FP32, or zero in one and
    not in the other. The loss gradient 2 (y - t) / (lum^2 + 0.01) of such a channel passes the gate in one numerics
    and not in another, so the row's whole contribution (large when the target is) appears or vanishes."""
    ym, y32 = oracle_forward(orc, kind, params, q, orc.MIXED), oracle_forward(orc, kind, params, q, orc.FP32)
    near = lambda y: (y > 0) & (y <= eps)  # noqa: E731
    return (near(ym) | near(y32) | ((ym > 0) != (y32 > 0))).any(axis=1)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def block_distances(orc, kind, params, q, t):
    """(g_mixed, loss_mixed, {block: rel-L2(MIXED, FP32)}): the oracle's own numerics error per parameter block, the
    yardstick of the per-block gradient bound max(2e-3, 2 d_block)"""
    g_m, loss = oracle_grad(orc, kind, params, q, t, orc.MIXED)
    g_32, _ = oracle_grad(orc, kind, params, q, t, orc.FP32)
    return g_m, loss, {k: rel_l2(g_m[i], g_32[i]) for k, i in case_blocks(kind).items()}
