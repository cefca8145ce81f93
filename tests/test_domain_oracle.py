"""The CPU oracle is fit to judge the GPU on the whole query domain (tests/domain_cases.py), checked without a GPU:

* its encoders (Frequency, padded, FrequencySH, Hash) against float64 restatements written here or in
  oracle/oracle_np.py, on the bulk and branch rows: 4e-6 absolute (the f32 evaluation error, as test_encode_parity), and
  exactly for the triangle wave of |x| > 1 (power-of-two scaling and u - floor(u) are exact there);
* every forward (MIXED, TCNN, FP32) and the MIXED gradient are finite, except on the listed rows whose Identity input
  rounds to f16 inf;
* the outlier cap of the GPU parity tests (0.1 % of the rows beyond 16 f16 ulps) is not used up by the oracle's own
  sensitivity: a one-ulp nudge of every position moves at most half that many rows that far;
* per parameter block, the oracle's own MIXED-vs-FP32 gradient distance on the domain batches, printed (DESIGN.md
  section 4 holds the table): the GPU gradient tests bound each block by max(2e-3, 2 x that distance).
"""
import numpy as np
import pytest

import domain_cases as dc
from oracle import oracle_np

N_INFER = dc.N_INFER


def _blob64(x):
    return oracle_np.encode(np.concatenate([np.zeros((len(x), 3)), x, np.zeros((len(x), 6))], axis=1))[:, 36:60]


def _sh64(theta, phi):
    x, y, z = np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    return np.stack([
        np.full_like(x, 0.28209479177387814), -0.48860251190291987 * y, 0.48860251190291987 * z,
        -0.48860251190291987 * x, 1.0925484305920792 * xy, -1.0925484305920792 * yz,
        0.94617469575755997 * z2 - 0.31539156525251999, -1.0925484305920792 * xz,
        0.54627421529603959 * (x2 - y2), 0.59004358992664352 * y * (-3.0 * x2 + y2), 2.8906114426405538 * xy * z,
        0.45704579946446572 * y * (1.0 - 5.0 * z2), 0.3731763325901154 * z * (5.0 * z2 - 3.0),
        0.45704579946446572 * x * (1.0 - 5.0 * z2), 1.4453057213202769 * z * (x2 - y2),
        0.59004358992664352 * x * (-x2 + 3.0 * y2)], axis=1)


def _hash64(table, pos):
    """tcnn GridEncoding in float64 from the formulas in oracle/nrc_hash_oracle.c's header: pos = scale x + 0.5 rounded
    to f32 once (the fmaf), cell = floor, trilinear weights, dense x + y res + z res^2 or x ^ y P1 ^ z P2 in uint32"""
    pos = np.asarray(pos, np.float64)
    out = np.zeros((len(pos), 32))
    off = 0
    for l in range(16):
        scale, res, entries = 16.0 * 2 ** l - 1.0, np.uint32(16 << l), 4096 if l == 0 else 32768
        p = (scale * pos + 0.5).astype(np.float32).astype(np.float64)
        fl = np.floor(p)
        fr = p - fl
        cell = (fl.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
        T = table[2 * off:2 * (off + entries)].reshape(entries, 2).astype(np.float64)
        for c in range(8):
            bit = [(c >> d) & 1 for d in range(3)]
            w = np.prod([fr[:, d] if bit[d] else 1.0 - fr[:, d] for d in range(3)], axis=0)
            g = [cell[:, d] + np.uint32(bit[d]) for d in range(3)]
            with np.errstate(over="ignore"):
                i = g[0] + g[1] * res + g[2] * res * res if l <= 1 else \
                    g[0] ^ (g[1] * np.uint32(2654435761)) ^ (g[2] * np.uint32(805459861))
            out[:, 2 * l:2 * l + 2] += w[:, None] * T[i & np.uint32(entries - 1)]
        off += entries
    return out


@pytest.fixture(scope="module")
def rows():
    return dc.domain_pool(), dc.domain_pool(hash_safe=True)


def test_generator_is_deterministic_and_covers_the_domain():
    q = dc.domain_pool()
    n = len(q)
    np.testing.assert_array_equal(q, dc.domain_queries(n))
    assert q.dtype == np.float32 and q.shape == (n, 15) and np.isfinite(q).all()
    assert not np.array_equal(q, dc.domain_queries(n, seed=dc.SEED + 1))
    # every branch row is among the rows the network-level tests use, but for the listed f16-overflow rows
    have = {r.tobytes() for r in dc.pool()}
    b = dc.branch_rows()
    assert all(r.tobytes() in have for r in b[~dc.f16_overflow_rows(b)])
    b = dc.bulk_rows(20000)
    inside = ((b[:, :3] >= 0) & (b[:, :3] < 1)).all(axis=1)
    assert 0.05 < 1.0 - inside.mean() < 0.2 and b[:, :3].min() < -0.15 and b[:, :3].max() > 1.15
    assert (b[:, [3, 5]] >= 0).all() and (b[:, [3, 5]] <= np.float32(np.pi)).all()
    assert (np.abs(b[:, [4, 6]]) <= np.float32(np.pi)).all() and (b[:, 7:] >= 0).all() and (b[:, 7:] <= 1).all()
    assert np.mean(b[:, 7:9] == 1.0) < 0.01 and np.mean(b[:, 12:15] == 0.0) < 0.01
    t = 4.0 * dc.blob_specials().astype(np.float64)
    assert {-5.0, -4.0, 7.0, 8.0} <= set(t.tolist())
    h = dc.domain_pool(hash_safe=True)
    assert np.abs(h[:, :3]).max() == dc.HASH_POS_MAX and np.abs(q[:, :3]).max() == 2.0 ** 20 + 0.5
    bad = dc.hostile_rows()
    assert (~np.isfinite(bad) | (np.abs(bad) >= 1e30)).any(axis=1).all()
    for cls in (dc.POS, dc.BLOB, dc.IDENT):
        assert np.isnan(bad[:, cls]).any() and np.isposinf(bad[:, cls]).any() and np.isneginf(bad[:, cls]).any()


def test_frequency_encoders_match_float64(orc, rows):
    q = rows[0]
    ref = oracle_np.encode(q)
    got = orc.encode(q)
    np.testing.assert_allclose(got, ref, rtol=0, atol=4e-6)
    big = np.repeat(np.abs(q[:, :3]) > 1.0, 12, axis=1)
    assert big.sum() > 1000
    np.testing.assert_array_equal(got[:, :36][big], ref[:, :36][big])
    # padded: the reference's column order with pad_ after the triangle wave (include/nrc/layout.h)
    pad = dc.pad_values(len(q))
    refp = np.concatenate([ref[:, :36], pad[:, None].astype(np.float64), ref[:, 36:66], np.ones((len(q), 13))], axis=1)
    np.testing.assert_allclose(orc.encode_padded(dc.padded(q, pad)), refp, rtol=0, atol=4e-6)
    # FrequencySH: SH of the direction, OneBlob of normal and roughness
    q64 = q.astype(np.float64)
    refs = np.concatenate([ref[:, :36], _sh64(q64[:, 3], q64[:, 4]), ref[:, 44:60], ref[:, 60:66],
                           np.ones((len(q), 6))], axis=1)
    np.testing.assert_allclose(orc.encode_sh(q), refs, rtol=0, atol=4e-6)
    np.testing.assert_array_equal(orc.encode_sh(q)[:, :36], got[:, :36])


def test_hash_encoder_matches_float64(orc, golden, rows):
    q = rows[1]
    params = dc.case_params("hash", orc, golden)
    got = orc.hash_encode(params, q, orc.FP32)
    ref = _hash64(params[orc.HASH_MLP_PARAMS:], q[:, :3])
    np.testing.assert_allclose(got[:, :32], ref, rtol=0, atol=4e-6)
    np.testing.assert_allclose(got[:, 32:62], oracle_np.encode(q)[:, 36:66], rtol=0, atol=4e-6)
    assert (got[:, 62:] == 1.0).all()
    # the dense levels see the whole table, not the few cells around the origin
    for l, entries in ((0, 4096), (1, 32768)):
        seen = {int(e) for r in q[:2000] for e in orc.hash_corners(r, l)[0]}
        assert len(seen) > 1000, (l, len(seen))
    # MIXED = the same corners and weights with f16 table, weights and FMA: within the f16 error of 8 terms of |T| <= 1
    mixed = orc.hash_encode(params, q, orc.MIXED)
    assert np.abs(mixed[:, :32] - ref).max() <= 8 * 2.0 ** -11


KINDS = ["frequency", "padded", "sh", "wide", "hash", "hash_padded"]


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_outputs_are_finite_except_listed_rows(orc, golden, rows, kind):
    """The listed rows are the only ones with a non-finite MIXED / TCNN output: the 6 with an Identity input of 65520
    (f16 inf) and the 6 with 65504, the largest f16 (its layer-0 products overflow the f16 hidden activations one layer
    on, dc.f16_overflow_rows). FP32 keeps every row finite. The listed rows stay out of every network-level comparison
    (dc.network_rows) and in the encoder-level ones."""
    h = kind.startswith("hash")
    q = rows[1] if h else rows[0]
    inf16 = (q[:, 9:15] == np.float32(65520.0)).any(axis=1)
    max16 = (q[:, 9:15] == np.float32(65504.0)).any(axis=1)
    with np.errstate(over="ignore"):
        np.testing.assert_array_equal(np.isinf(q[:, 9:15].astype(np.float16)).any(axis=1), inf16)
    listed = inf16 | max16
    np.testing.assert_array_equal(dc.f16_overflow_rows(q), listed)
    assert inf16.sum() == 6 and max16.sum() >= 6
    params = dc.case_params(kind, orc, golden)
    qk = dc.padded(q, dc.pad_values(len(q))) if kind.endswith("padded") else q
    for mode in (orc.MIXED, orc.TCNN, orc.FP32):
        y = dc.oracle_forward(orc, kind, params, qk, mode)
        bad = ~np.isfinite(y).all(axis=1)
        print(f"{kind} mode {mode}: non-finite rows {int(bad.sum())} ({int((bad & inf16).sum())} of the 65520 rows, "
              f"{int((bad & max16 & ~inf16).sum())} of the 65504 rows)")
        assert not bad[~listed].any(), (mode, np.flatnonzero(bad & ~listed)[:5], qk[bad & ~listed][:2])
        if mode == orc.FP32:
            assert not bad.any()
    np.testing.assert_array_equal(dc.network_rows(q, h), q[~listed])


@pytest.mark.parametrize("kind", ["frequency", "sh", "padded", "wide", "hash", "hash_padded"])
def test_outlier_cap_is_not_spent_by_the_oracle(orc, golden, kind):
    """The GPU parity tests allow 0.1 % of N_INFER rows beyond 16 f16 ulps of their scale (the top octave's slope is
    2 x 2^11). Here: the rows the MIXED oracle itself moves that far when every position is nudged by one f32 ulp; at
    most half the cap (8 of 16,385 rows).

    With weights of one magnitude in every octave / level the oracle moves 0.2 % - 0.9 % of the rows (Hash: half of
    them), whatever the seed or the row count; the domain tests' weights are scaled per octave / level for that reason
    (dc.damp_octaves, dc.case_params; figures in DESIGN.md section 4)."""
    q = dc.case_queries(kind, N_INFER)
    params = dc.case_params(kind, orc, golden)
    y = dc.oracle_forward(orc, kind, params, q, orc.MIXED)
    moved = 0
    for toward in (np.inf, -np.inf):
        qn = q.copy()
        qn[:, :3] = np.nextafter(q[:, :3], np.float32(toward))
        yn = dc.oracle_forward(orc, kind, params, qn, orc.MIXED)
        tol = 16.0 * 2.0 ** -11 * np.maximum(np.abs(y).max(axis=1), 1e-2)
        far = np.abs(yn - y).max(axis=1) > tol
        print(f"{kind}: one ulp toward {toward}: {int(far.sum())} of {N_INFER} rows beyond 16 ulps, e.g. {q[far][:3, :3]}")
        moved = max(moved, int(far.sum()))
    assert moved <= 0.5 * 0.001 * N_INFER, moved


@pytest.mark.parametrize("kind,b", dc.GRAD_CASES)
def test_oracle_gradient_blocks(orc, golden, nrc, kind, b):
    """Finite MIXED gradient and loss on the domain batch; prints d_block = rel-L2(MIXED, FP32) per parameter block."""
    q = dc.train_queries(kind, b)
    t = dc.train_targets(nrc, b)
    g, loss, d = dc.block_distances(orc, kind, dc.case_params(kind, orc, golden), q, t)
    assert np.isfinite(g).all() and np.isfinite(loss)
    print(f"{kind} b={b}: loss {loss:.6g}; d_block " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
    assert all(np.isfinite(v) for v in d.values())
    blocks = dc.case_blocks(kind)
    if kind != "hash":  # the blocks partition the blob
        assert sorted(np.concatenate(list(blocks.values())).tolist()) == list(range(g.size))
    else:
        for l in (0, 1):
            sl = blocks[f"grid.L{l}"]
            assert np.count_nonzero(g[sl].reshape(-1, 2).any(axis=1)) > 1000
