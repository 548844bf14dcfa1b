"""-m gpu: the narrow stream's eight slice bodies (one to four groups of four transcripts x bytes contiguous in the ring or
wrapping around its end) and what the loop keeps per RUN of slices with one transcript set -- the x rows, the gradient rows'
addresses spread for the flush, the sums in registers -- on small samples built by hand:

  * transcript sets of 4, 5, 8, 9, 12, 13 and 16 transcripts, each in runs of one, two and six slices of 64 identical sets, a
    run of 26 slices (longer than a wave's share of a 64-slice tile, so it is cut between two waves), and a run whose last
    slice is a zero-padded remainder; a tile's slices are ordered by set size, so runs change in the middle of every wave's
    share, and a wave's share (sixteen slices of 1.25 .. 4.25 KiB) passes the 7 KiB ring several times: slices wrap;
  * the masked variant adds leftover rows: 2 .. 5 transcripts of a union of 16, a different subset per fragment, one union per
    block of 256 transcripts so that masked slices come in runs (stream A1M; a union of 11 becomes zero-padded dense slices);
  * with multiplicities, and at K = 1, 4, 6 and 8 draws (one and two draw groups).

Check 1: gradient and lp against the float64 oracle at the tolerances of tests/test_gpu_stream_kernel_oracle.py (lp 1e-6
relative; gradient 1e-4 relative + 1e-6 of the largest entry), for the instances that return lp and for the gradient-only
instances (the VI step's).  Check 2: in deterministic mode the library built with the backend tuning flags and the one built
without them return the same bits."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import ROOT
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N = 560
WIDTHS = (4, 5, 8, 9, 12, 13, 16)
RUN_SLICES = (1, 2, 6)
LONG_RUN = (9, 26)      # (transcripts, slices): longer than a wave's share of a tile
REMAINDER = (16, 3, 40)  # (transcripts, whole slices, rows of the zero-padded last slice)
UNIONS, UNION_ROWS = (16, 11, 16), 256  # transcripts of each union; leftover rows per union
VARIANTS = ("dense", "masked", "ks")
DRAWS = (1, 4, 6, 8)


def make_rows(variant):
    """[(sorted 0-based transcript ids, values)] per fragment, in random order; the multiplicities or None."""
    rng = np.random.default_rng(20240 + VARIANTS.index(variant))
    free = list(rng.permutation(N))

    def new_set(w, bin256=None):  # (bin256: all from transcripts 256 bin256 .. 256 bin256 + 255)
        take = [t for t in free if bin256 is None or t // 256 == bin256][:w]
        for t in take:
            free.remove(t)
        return np.sort(np.array(take))

    rows = []

    def add_run(cols, nrows):
        for _ in range(nrows):
            rows.append((cols, rng.uniform(0.05, 1.0, len(cols)).astype(np.float32)))

    if variant != "dense":
        # (the rows' sort key starts with the first transcript's block of 256: a union per block keeps its leftover rows together,
        # so that masked slices with one union follow each other)
        for u, wu in enumerate(UNIONS):
            union = new_set(wu, u)
            for _ in range(UNION_ROWS):
                sub = np.sort(rng.choice(union, int(rng.integers(2, 6)), replace=False))
                rows.append((sub, rng.uniform(0.05, 1.0, len(sub)).astype(np.float32)))
    for w in WIDTHS:
        for r in RUN_SLICES:
            add_run(new_set(w), 64 * r)
    add_run(new_set(LONG_RUN[0]), 64 * LONG_RUN[1])
    add_run(new_set(REMAINDER[0]), 64 * REMAINDER[1] + REMAINDER[2])
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    ks = rng.integers(1, 6, len(rows)).astype(np.int64) if variant == "ks" else None
    return rows, ks


def to_csc(rows):
    """colptr (1-based, uint64), rowval (1-based, ascending inside a column), nzval"""
    r = np.concatenate([np.full(len(c), i, np.int64) for i, (c, _) in enumerate(rows)])
    c = np.concatenate([c for c, _ in rows]).astype(np.int64)
    v = np.concatenate([v for _, v in rows])
    o = np.lexsort((r, c))
    colptr = np.ones(N + 1, np.uint64)
    colptr[1:] += np.cumsum(np.bincount(c, minlength=N)).astype(np.uint64)
    return colptr, (r[o] + 1).astype(np.uint32), v[o]


def draws(K):
    x = np.random.default_rng(K).gamma(0.3, size=(K, N)).astype(np.float32) + np.float32(1e-7)
    x /= x.sum(axis=1, keepdims=True)
    return np.clip(x, np.float32(1e-10), 1)


_inputs = {}


def inputs(variant):
    if variant not in _inputs:
        rows, ks = make_rows(variant)
        _inputs[variant] = (len(rows),) + to_csc(rows) + (ks,)
    return _inputs[variant]


def gpu_sample(P, variant, ctx):
    m, colptr, rowval, nzval, ks = inputs(variant)
    return P.RNASeqSample(m, N, colptr, rowval, nzval, np.ones(N, np.float32), ks=ks, ctx=ctx)


@pytest.fixture(scope="module")
def P():
    import polee_amd
    return polee_amd


@pytest.fixture(scope="module")
def reference():
    """(variant, K) -> (lp [K], gradient [K, n]) of the float64 oracle, computed once"""
    cache = {}

    def get(variant, K):
        if (variant, K) not in cache:
            m, colptr, rowval, nzval, ks = inputs(variant)
            so = O.Sample(m, N, colptr, rowval, nzval)
            x = draws(K)
            res = [so.log_likelihood(x[k]) if ks is None else so.factored_log_likelihood(ks, x[k]) for k in range(K)]
            cache[(variant, K)] = (np.array([r[0] for r in res]), np.stack([r[1] for r in res]))
        return cache[(variant, K)]

    return get


def check_gradient(g, go, what):
    for k in range(go.shape[0]):
        scale = np.abs(go[k]).max()
        print("%s draw %d: worst weighted gradient err %.3g" % (what, k, float((np.abs(g[k] - go[k]) / (np.abs(go[k]) + 1e-2 * scale)).max())))
        np.testing.assert_allclose(g[k], go[k], rtol=1e-4, atol=1e-6 * scale)


@pytest.mark.parametrize("K", DRAWS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_runs_of_every_narrow_body_match_the_oracle(P, reference, variant, K):
    ctx = P.Context(0)
    s = gpu_sample(P, variant, ctx)
    tiles = list(s.info["stream_tiles"])[:6]
    print("tiles per stream (A1, A1M, A2, A2M, BN, B):", tiles)
    assert tiles[0] >= 2, tiles                        # dense narrow: more than one tile
    assert (tiles[1] > 0) == (variant != "dense"), tiles  # masked narrow: the leftover rows
    assert tiles[2] == tiles[3] == tiles[5] == 0, tiles
    lpo, go = reference(variant, K)
    x = draws(K)
    lp, g = s.log_likelihood(x)
    for k in range(K):
        err = abs(lp[k] - lpo[k]) / abs(lpo[k])
        print("%s K=%d draw %d: lp rel err %.3g" % (variant, K, k, err))
        assert err <= 1e-6, (variant, K, k, lp[k], lpo[k])
    check_gradient(g, go, "%s K=%d" % (variant, K))
    _, g2 = s.log_likelihood(x, gradonly=True)  # the instances without lp: four waves per SIMD, other register allocation
    check_gradient(g2, go, "%s K=%d gradient only" % (variant, K))


CODE = textwrap.dedent("""
    import sys
    sys.path[:0] = [%r, %r]
    import numpy as np
    import polee_amd as P
    from polee_amd import _lib as L
    import test_gpu_stream_runs as T
    res = {"version": L.lib().polee_version().decode()}
    ctx = P.Context(0)
    for variant in T.VARIANTS:
        s = T.gpu_sample(P, variant, ctx)
        s.set_deterministic(True)
        for K in T.DRAWS:
            x = T.draws(K)
            res["%%s_%%d_lp" %% (variant, K)], res["%%s_%%d_g" %% (variant, K)] = s.log_likelihood(x)
            res["%%s_%%d_gonly" %% (variant, K)] = s.log_likelihood(x, gradonly=True)[1]
        del s
    np.savez(sys.argv[1], **res)
""") % (ROOT, os.path.join(ROOT, "tests"))


def _run(lib, out):
    env = dict(os.environ)
    if lib:
        env["POLEE_HIP_LIB"] = lib
    r = subprocess.run([sys.executable, "-c", CODE, out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(out)


def test_tuned_and_untuned_builds_agree_bit_for_bit_on_runs(tmp_path):
    untuned = os.path.join(ROOT, "polee_amd", "csrc", "libpolee_hip_untuned.so")
    assert os.path.exists(untuned), "libpolee_hip_untuned.so is not built (make -C polee_amd/csrc untuned)"
    a = _run(None, str(tmp_path / "tuned.npz"))
    b = _run(untuned, str(tmp_path / "untuned.npz"))
    assert "gate build" in str(b["version"]) and "gate build" not in str(a["version"])
    keys = [k for k in a.files if k != "version"]
    assert len(keys) == 3 * len(VARIANTS) * len(DRAWS)
    for key in keys:
        assert np.array_equal(a[key], b[key]), key
        assert np.isfinite(a[key]).all(), key
