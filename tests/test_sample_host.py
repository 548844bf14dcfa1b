"""CPU tests of `polee sample`'s host side (polee_amd.sample; no GPU): a NumPy restatement of the arithmetic csrc/sample.hip fixes
(props, posterior mean, expected counts), a NumPy restatement of the multinomial splitting construction with the two statistics that
judge it (pooled chi-square, dispersion), and the two writers fed from NumPy batches.  tests/test_gpu_sample.py imports the
restatements and the statistics and applies them to the device's output."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy import stats

from conftest import GOLDEN

PREP_H5 = os.path.join(GOLDEN, "mBr_M_6w_1.prep.h5")
FIXTURE_M = 19743


# ---- the arithmetic of DESIGN.md section 3.9, restated ----------------------------------------------------------------------------
def restate_props(raw, efflens):
    """t = x / l in f32 (one rounding, as xs ./= efflens); S = sum t in f64; prop = (float)((double)t / S)."""
    raw = np.asarray(raw, np.float32).reshape(-1, np.size(efflens))
    t = raw / np.asarray(efflens, np.float32)[None, :]
    assert t.dtype == np.float32
    S = t.astype(np.float64).sum(axis=1)
    return (t.astype(np.float64) / S[:, None]).astype(np.float32)


def restate_posterior_mean(props):
    """f64 accumulation per transcript in draw order, handed out as f32."""
    props = np.asarray(props, np.float32)
    acc = np.zeros(props.shape[1], np.float64)
    for row in props:
        acc += row.astype(np.float64)
    return (acc / props.shape[0]).astype(np.float32)


def restate_expected_counts(prop, efflens, m):
    """expected_counts (main.jl:859-863) entirely in f64: e = prop * l, counts = e / sum(e) * m."""
    e = np.asarray(prop, np.float32).astype(np.float64) * np.asarray(efflens, np.float32).astype(np.float64)
    return e / e.sum(axis=-1, keepdims=True) * float(m)


# ---- the splitting construction, restated, and its judges ---------------------------------------------------------------------------
def heavy_tailed_shares(n=313, seed=20260117):
    """One fixed share vector like a draw of the fixture's approximation: a dominant transcript at 0.6, the bulk log-uniform over
    seven decades below it, one transcript at 1e-10; normalised.  (The spread is chosen, before any sampler was run, so that the
    dispersion test below has at least 10 categories to look at for m = 19 743 and at least 150 for m = 30 M: it has 39 and 170.)"""
    rng = np.random.default_rng(seed)
    rest = np.exp(rng.uniform(np.log(1e-8), np.log(0.25), n - 1))
    rest[0] = 1e-10 * rest[1:].sum() / 0.4
    p = np.concatenate([[0.6], 0.4 * rest / rest.sum()])
    p = p[rng.permutation(n)]
    return p / p.sum()


def split_levels(n):
    L = 0
    while (1 << L) < n:
        L += 1
    return L


def restate_multinomial_by_splitting(p, m, D, rng):
    """D multinomial draws of m items by the construction of csrc/sample.hip: the count m at the root of a balanced binary tree over
    the categories; node i of level lev covers [i n / 2^lev, (i+1) n / 2^lev) and hands Binomial(c, mass of its first half / its
    mass) to child 2i, the rest to child 2i + 1.  numpy.random.Generator.binomial at the nodes."""
    p = np.asarray(p, np.float64)
    n = p.size
    P = np.concatenate([[0.0], np.cumsum(p)])
    L = split_levels(n)
    c = np.full((D, 1), int(m), np.int64)
    for lev in range(L):
        i = np.arange(1 << lev, dtype=np.int64)
        lo, hi, mid = (i * n) >> lev, ((i + 1) * n) >> lev, ((2 * i + 1) * n) >> (lev + 1)
        wl, w = P[mid] - P[lo], P[hi] - P[lo]
        q = np.where(w > 0, wl / np.where(w > 0, w, 1.0), 0.0)
        q = np.where(mid <= lo, 0.0, np.where(hi <= mid, 1.0, np.clip(q, 0.0, 1.0)))
        left = rng.binomial(c, q[None, :])
        nxt = np.empty((D, 2 << lev), np.int64)
        nxt[:, 0::2] = left
        nxt[:, 1::2] = c - left
        c = nxt
    i = np.arange(1 << L, dtype=np.int64)
    lo, hi = (i * n) >> L, ((i + 1) * n) >> L
    out = np.zeros((D, n), np.int64)
    out[:, lo[hi > lo]] = c[:, hi > lo]
    assert (c[:, hi <= lo] == 0).all()
    return out


def pooled_chi2(counts, p, m):
    """Draw totals against D m p; categories with an expected total below 10 are pooled into one.  -> (chi2, df, limit at 1e-9)."""
    counts = np.asarray(counts)
    D = counts.shape[0]
    p = np.asarray(p, np.float64) / np.sum(p)
    expect = D * float(m) * p
    obs = counts.sum(axis=0).astype(np.float64)
    small = expect < 10.0
    e = np.concatenate([expect[~small], [expect[small].sum()]]) if small.any() else expect
    o = np.concatenate([obs[~small], [obs[small].sum()]]) if small.any() else obs
    if e[-1] == 0.0:
        assert o[-1] == 0.0
        e, o = e[:-1], o[:-1]
    chi = float(((o - e) ** 2 / e).sum())
    df = e.size - 1
    return chi, df, float(stats.chi2.isf(1e-9, df))


def dispersion(counts, p, m):
    """Per category with m p (1 - p) >= 50: sum_d (c_dj - m p_j)^2 / (m p_j (1 - p_j)), chi-square with D degrees of freedom under
    the multinomial.  -> (statistics, low, high, categories tested); the window leaves 1e-9 / categories outside, half on each
    side."""
    counts = np.asarray(counts, np.float64)
    D = counts.shape[0]
    p = np.asarray(p, np.float64) / np.sum(p)
    var = float(m) * p * (1.0 - p)
    take = var >= 50.0
    k = int(take.sum())
    if k == 0:
        return np.zeros(0), 0.0, np.inf, 0
    s = ((counts[:, take] - float(m) * p[take]) ** 2 / var[take]).sum(axis=0)
    a = 1e-9 / k
    return s, float(stats.chi2.ppf(a / 2, D)), float(stats.chi2.isf(a / 2, D)), k


def check_multinomial(counts, p, m, min_categories):
    counts = np.asarray(counts)
    assert (counts.sum(axis=1) == m).all()
    chi, df, limit = pooled_chi2(counts, p, m)
    s, lo, hi, k = dispersion(counts, p, m)
    print("m = %d, D = %d: pooled chi2 %.1f (df %d, limit %.1f); dispersion over %d categories in [%.1f, %.1f], window [%.1f, %.1f]"
          % (m, counts.shape[0], chi, df, limit, k, s.min() if k else 0, s.max() if k else 0, lo, hi))
    assert chi < limit, (chi, df, limit)
    assert k >= min_categories, k
    assert (s > lo).all() and (s < hi).all(), (s.min(), s.max(), lo, hi)
    return chi, k


def test_restated_arithmetic_identities():
    rng = np.random.default_rng(5)
    n, D, m = 313, 12, FIXTURE_M
    raw = rng.dirichlet(np.full(n, 0.05), size=D).astype(np.float32) + np.float32(1e-16)
    l = rng.uniform(50.0, 4000.0, n).astype(np.float32)
    props = restate_props(raw, l)
    assert props.dtype == np.float32 and props.shape == (D, n)
    np.testing.assert_allclose(props.astype(np.float64).sum(axis=1), 1.0, rtol=0, atol=n * 2.0 ** -24)
    counts = restate_expected_counts(props, l, m)
    assert counts.dtype == np.float64
    np.testing.assert_allclose(counts.sum(axis=1), m, rtol=1e-12, atol=0)
    # expected counts undo the effective-length adjustment: proportional to the raw draw (to the f32 roundings of t and prop)
    ratio = counts / raw.astype(np.float64)
    np.testing.assert_allclose(ratio, ratio[:, :1] * np.ones((1, n)), rtol=4 * 2.0 ** -24)
    pm = restate_posterior_mean(props)
    assert pm.dtype == np.float32
    np.testing.assert_allclose(pm, props.astype(np.float64).mean(axis=0), rtol=2.0 ** -23)
    ec = restate_expected_counts(pm, l, m)
    np.testing.assert_allclose(ec.sum(), m, rtol=1e-12)
    assert restate_expected_counts(pm, l, 0).max() == 0.0


@pytest.mark.parametrize("m,min_categories", [(FIXTURE_M, 10), (30_000_000, 150)])
def test_helpers_accept_numpy_multinomial_and_the_restated_splitting(m, min_categories):
    p = heavy_tailed_shares()
    assert p.size == 313 and p.min() < 1.1e-10 and 0.55 < p.max() < 0.65 and abs(p.sum() - 1) < 1e-12
    for D in (256, 1024):
        ref = np.random.default_rng(100 + D).multinomial(m, p, size=D)
        check_multinomial(ref, p, m, min_categories)
        got = restate_multinomial_by_splitting(p, m, D, np.random.default_rng(200 + D))
        check_multinomial(got, p, m, min_categories)


def test_helpers_reject_wrong_samplers():
    """The judges have teeth: overdispersed counts, underdispersed counts and a biased share all fail."""
    p, m, D = heavy_tailed_shares(), 30_000_000, 1024
    rng = np.random.default_rng(9)
    good = rng.multinomial(m, p, size=D)
    # overdispersed: every draw uses shares perturbed by 0.1 %
    def perturbed():
        q = p * np.exp(rng.normal(0, 1e-3, p.size))
        return q / q.sum()
    over = np.stack([rng.multinomial(m, perturbed()) for _ in range(D)])
    s, lo, hi, k = dispersion(over, p, m)
    assert k >= 150 and (s > hi).any()
    # biased: one mid-sized category gets 1 % more than its share
    j = int(np.argsort(p)[-20])
    q = p.copy(); q[j] *= 1.01; q /= q.sum()
    chi, df, limit = pooled_chi2(rng.multinomial(m, q, size=D), p, m)
    assert chi > limit
    # underdispersed: the same draw repeated with its rounding noise only
    s, lo, hi, k = dispersion(np.repeat(np.round(m * p)[None, :], D, axis=0), p, m)
    assert (s < lo).all()
    check_multinomial(good, p, m, 150)


def test_splitting_tree_partitions_the_categories():
    for n in (1, 2, 3, 5, 64, 313, 1000, 4097):
        L = split_levels(n)
        i = np.arange(1 << L, dtype=np.int64)
        lo, hi = (i * n) >> L, ((i + 1) * n) >> L
        assert ((hi - lo) <= 1).all() and sorted(lo[hi > lo].tolist()) == list(range(n))
        for lev in range(L):
            k = np.arange(1 << lev, dtype=np.int64)
            a, b, c = (k * n) >> lev, ((2 * k + 1) * n) >> (lev + 1), ((k + 1) * n) >> lev
            assert (a <= b).all() and (b <= c).all() and (np.abs((b - a) - (c - b)) <= 1).all()
    out = restate_multinomial_by_splitting(np.array([0.0, 1.0, 0.0, 3.0, 0.0]), 1000, 50, np.random.default_rng(1))
    assert (out.sum(axis=1) == 1000).all() and (out[:, [0, 2, 4]] == 0).all()
    assert abs(out[:, 3].mean() - 750) < 7 * np.sqrt(1000 * 0.1875 / 50)


# ---- writers ------------------------------------------------------------------------------------------------------------------------
def _batches(rng, n, sizes):
    return [rng.uniform(0, 100, (b, n)) for b in sizes]


def test_kallisto_writer_layout(tmp_path):
    from polee_amd import h5io
    from polee_amd.sample import write_kallisto
    rng = np.random.default_rng(3)
    n, sizes = 17, [4, 4, 3]
    N = sum(sizes)
    l = rng.uniform(100, 2000, n).astype(np.float32)
    props = restate_props(rng.dirichlet(np.ones(n), size=N).astype(np.float32), l)
    counts = restate_expected_counts(props, l, 5000)
    pm = restate_posterior_mean(props)
    ids = ["ENST%05d.1" % j for j in range(n)]
    lens = np.arange(1000, 1000 + n)
    consumed = []

    def gen():
        k = 0
        for b in sizes:
            consumed.append(k)
            yield counts[k:k + b]
            k += b

    def est():
        assert consumed == [0, 4, 8]  # evaluated after the batches: the posterior mean is known only then
        return restate_expected_counts(pm, l, 5000)

    fn = str(tmp_path / "k.h5")
    assert write_kallisto(fn, gen(), est, l, ids, lens, call="prep.h5 --kallisto") == N
    with h5io.File(fn) as f:
        kinds = {name: f.dataset_kind(name) for name in
                 ("est_counts", "aux/num_bootstrap", "aux/eff_lengths", "aux/lengths", "aux/ids", "aux/call", "aux/index_version",
                  "aux/kallisto_version", "aux/start_time")}
        assert kinds["est_counts"] == ("float", 8, (n,))
        assert kinds["aux/num_bootstrap"] == ("integer", 8, (1,))
        assert kinds["aux/eff_lengths"] == ("float", 8, (n,))
        assert kinds["aux/lengths"] == ("integer", 8, (n,))
        assert kinds["aux/ids"][0] == "string" and kinds["aux/ids"][2] == (n,)
        assert kinds["aux/call"][0] == "string" and kinds["aux/call"][2] == (1,)
        assert kinds["aux/index_version"] == ("integer", 8, (1,))
        assert kinds["aux/kallisto_version"][0] == "string" and kinds["aux/kallisto_version"][2] == ()
        assert kinds["aux/start_time"][0] == "string" and kinds["aux/start_time"][2] == ()
        assert f.read("aux/num_bootstrap", np.int64).tolist() == [N]
        assert f.read("aux/index_version", np.int64).tolist() == [-1]
        assert f.read_strings("aux/kallisto_version") == "polee sample"
        assert f.read_strings("aux/ids") == ids
        assert f.read_strings("aux/call") == ["prep.h5 --kallisto"]
        np.testing.assert_array_equal(f.read("aux/lengths", np.int64), lens)
        np.testing.assert_array_equal(f.read("aux/eff_lengths", np.float64), l.astype(np.float64))
        np.testing.assert_array_equal(f.read("est_counts", np.float64), restate_expected_counts(pm, l, 5000))
        for k in range(N):
            assert f.dataset_kind("bootstrap/bs%d" % k) == ("float", 8, (n,))
            np.testing.assert_array_equal(f.read("bootstrap/bs%d" % k, np.float64), counts[k])
        assert not f.exists("bootstrap/bs%d" % N)
    # est_counts as an array; wrong shapes are errors
    assert write_kallisto(fn, [counts[:2]], counts[0], l, ids, lens) == 2
    with pytest.raises(ValueError):
        write_kallisto(fn, [counts[:2, :-1]], counts[0], l, ids, lens)
    with pytest.raises(ValueError):
        write_kallisto(fn, [counts[:2]], counts[0], l, ids[:-1], lens)


def test_csv_writer(tmp_path):
    from polee_amd.sample import write_csv
    pm = np.array([0.25, 1e-9, 0.5, 3.3e-5], np.float32)
    fn = str(tmp_path / "s.csv")
    write_csv(fn, pm, ["a", "b", "c", "d"])
    lines = open(fn).read().split("\n")
    assert lines[0] == "transcript_id,tpm" and lines[-1] == "" and len(lines) == 6
    for line, tid, v in zip(lines[1:], "abcd", pm):
        name, val = line.split(",")
        assert name == tid and float(val) == 1e6 * float(v)  # the Float64 product of the Float32 mean, round-trip exact
    with pytest.raises(ValueError):
        write_csv(fn, pm, ["a"])


def test_default_names_and_command_line():
    from polee_amd import sample
    assert sample.default_output_filename(True) == "polee-sample.h5"
    assert sample.default_output_filename(False) == "polee-sample.csv"
    doc = sample.__doc__
    for flag in ("--kallisto", "--num-samples", "--sample-counts", "--transformation", "--trim-prefix", "--seed", "--transcript-ids",
                 "--transcript-lengths", "--batch"):
        assert flag in doc
    assert "--uniform-gene-prior" in doc  # (named as left out)
    with pytest.raises(SystemExit):
        sample.main(["--annotations", "x.gff", "prep.h5"])  # not offered


def test_names_trim_prefix_and_transformation_ids(tmp_path):
    from polee_amd import h5io
    from polee_amd.sample import resolve_names
    ids, lens = resolve_names(3)
    assert ids == ["1", "2", "3"] and lens.tolist() == [-1, -1, -1] and lens.dtype == np.int64
    ids, lens = resolve_names(3, ["transcript:A", "transcript:B", "C"], [10, 20, 30], trim_prefix="transcript:")
    assert ids == ["A", "B", "C"] and lens.tolist() == [10, 20, 30]
    with pytest.raises(ValueError):
        resolve_names(3, ["a", "b"])
    with pytest.raises(ValueError):
        resolve_names(3, None, [1, 2])
    # a transformation file: its transcript_ids win over the caller's (main.jl:776-779); fixed-length strings ...
    fn = str(tmp_path / "t.h5")
    with h5io.File(fn, "w") as f:
        f.write("node_parent_idxs", np.array([0, 1, 1, 2, 2], np.int32))
        f.write("node_js", np.array([0, 0, 1, 2, 3], np.int32))
        f.write_strings("transcript_ids", ["pre-x", "pre-yy", "z"])
    assert h5io.read_transformation_ids(fn) == ["pre-x", "pre-yy", "z"]
    parents, js = h5io.read_transformation(fn)  # (unchanged: the two arrays)
    assert parents.tolist() == [0, 1, 1, 2, 2] and js.tolist() == [0, 0, 1, 2, 3]
    assert resolve_names(3, ["a", "b", "c"], transformation=fn, trim_prefix="pre-")[0] == ["x", "yy", "z"]
    with pytest.raises(ValueError):
        resolve_names(4, transformation=fn)
    # ... and variable-length ones, as HDF5.jl writes an Array{String}
    fv = str(tmp_path / "v.h5")
    H = h5io.lib()
    hid = h5io.hid_t
    with h5io.File(fv, "w") as f:
        t = H.H5Tcopy(hid(h5io._g("H5T_C_S1_g")))
        H.H5Tset_size(hid(t), C.c_size_t(h5io.H5T_VARIABLE))
        H.H5Tset_cset(hid(t), h5io.H5T_CSET_UTF8)
        sp = H.H5Screate_simple(1, (C.c_uint64 * 1)(3), None)
        d = H.H5Dcreate2(hid(f.id), b"transcript_ids", hid(t), hid(sp), hid(0), hid(0), hid(0))
        assert d >= 0
        buf = (C.c_char_p * 3)(b"ENST1", b"a-much-longer-transcript-name", b"")
        assert H.H5Dwrite(hid(d), hid(t), hid(0), hid(0), hid(0), buf) >= 0
        H.H5Dclose(hid(d)); H.H5Sclose(hid(sp)); H.H5Tclose(hid(t))
    assert h5io.read_transformation_ids(fv) == ["ENST1", "a-much-longer-transcript-name", ""]
    with h5io.File(str(tmp_path / "none.h5"), "w") as f:
        f.write("node_js", np.array([1], np.int32))
    with pytest.raises(h5io.HDF5Error):
        h5io.read_transformation_ids(str(tmp_path / "none.h5"))


def test_errors_raised_before_any_device_work(tmp_path, monkeypatch):
    """An ids list whose length is not n, and a prepared sample of another format version: both fail on the host."""
    from polee_amd import h5io
    from polee_amd.sample import polee_sample
    with pytest.raises(ValueError, match="313"):
        polee_sample(PREP_H5, str(tmp_path / "o.csv"), transcript_ids=["a", "b"])
    ps = h5io.read_prepared_sample(PREP_H5)
    old = str(tmp_path / "old.h5")
    monkeypatch.setattr(h5io, "PREPARED_SAMPLE_FORMAT_VERSION", h5io.PREPARED_SAMPLE_FORMAT_VERSION - 1)
    h5io.write_approximation(old, ps["m"], ps["n"], ps["effective_lengths"], ps)
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="older version"):
        polee_sample(old, str(tmp_path / "o.csv"))
    with pytest.raises(ValueError):
        polee_sample(PREP_H5, str(tmp_path / "o.csv"), num_samples=0)
    assert not os.path.exists(str(tmp_path / "o.csv"))


def test_package_exports():
    import polee_amd
    from polee_amd import sample
    assert polee_amd.polee_sample is sample.polee_sample
    assert polee_amd.ApproxSampleStream is sample.ApproxSampleStream
    assert polee_amd.multinomial_counts is sample.multinomial_counts
    assert callable(sample.main) and callable(sample.write_kallisto) and callable(sample.write_csv)
