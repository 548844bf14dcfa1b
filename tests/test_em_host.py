"""EM maximum-likelihood estimate (polee_amd.em; `polee debug-optimize`, src/em.jl): a NumPy restatement of em.jl -- in f64, and in
f32 as the device computes (f32 products, row sums, reciprocals and updates) -- checked against closed forms and a brute-force
maximum; the CSV writer and the CLI's argument checks.  No GPU.  tests/test_gpu_em.py imports the restatement."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT  # noqa: F401
from test_gibbs_host import rows_of

import polee_amd.em as E

FIXTURE_MAX = -326994.3908  # lp of the f64 restatement after 3 000 iterations (SURVEY.md's -326 994.4)


class Problem:
    """X by rows (indptr, col 0-based ascending, val f32) with optional multiplicities; empty rows are dropped as the device
    layout drops them."""

    def __init__(self, m, n, indptr, col, val, ks=None):
        lens = np.diff(indptr)
        self.m, self.n = int(m), int(n)
        self.keep = np.flatnonzero(lens > 0)
        self.starts = np.asarray(indptr[:-1], np.int64)[self.keep]
        self.col = np.asarray(col, np.int64)
        self.val32 = np.asarray(val, np.float32)
        self.row = np.repeat(np.arange(self.keep.size), lens[self.keep])
        self.ks = np.ones(self.keep.size) if ks is None else np.asarray(ks, np.float64)[self.keep]
        self.M = float(self.ks.sum())
        # entries by transcript, for f32 sums in a fixed order
        self.by_col = np.argsort(self.col, kind="stable")
        self.col_starts = np.flatnonzero(np.diff(np.concatenate([[-1], self.col[self.by_col]])))
        self.cols_present = self.col[self.by_col][self.col_starts]

    @classmethod
    def from_csc(cls, lm, ks=None):
        return cls(lm["m"], lm["n"], *rows_of(lm["m"], lm["n"], lm["colptr"], lm["rowval"], lm["nzval"]), ks=ks)

    def frag_probs(self, y, dtype=np.float64):
        w = self.val32.astype(dtype) * np.asarray(y, dtype)[self.col]
        return w, np.add.reduceat(w, self.starts) if w.size else np.zeros(0, dtype)

    def lp64(self, y):
        """sum_i ks_i log sum_j X_ij y_j in f64, of y as given (normalise first)."""
        _, p = self.frag_probs(np.asarray(y, np.float64))
        with np.errstate(divide="ignore"):
            return float((self.ks * np.log(p)).sum())

    def gradient(self, y, dtype=np.float64):
        """g_j = sum_i ks_i X_ij / p_i; in f32 every term and every running sum is an f32."""
        _, p = self.frag_probs(y, dtype)
        c = self.val32.astype(dtype) * (self.ks.astype(dtype) * (dtype(1) / p))[self.row]
        if dtype is np.float64:
            return np.bincount(self.col, weights=c, minlength=self.n)
        g = np.zeros(self.n, dtype)
        if c.size:
            g[self.cols_present] = np.add.reduceat(c[self.by_col], self.col_starts)
        return g

    def step(self, y, dtype=np.float64):
        """One iteration of em.jl:42-69 as y <- y g / M (the same numbers: cs_j = y_j g_j, cs_sum = M)."""
        return (np.asarray(y, dtype) * self.gradient(y, dtype) * dtype(1.0 / self.M)).astype(dtype)


def run_em(P, iters, dtype=np.float64, y0=None, trace=True):
    """iters iterations from 1/n (em.jl:22) or y0; returns (y normalised in f64, lp64 of iterates 1..iters)."""
    y = np.full(P.n, 1.0 / P.n, dtype) if y0 is None else (np.asarray(y0, np.float64) / np.sum(y0, dtype=np.float64)).astype(dtype)
    lps = []
    for _ in range(iters):
        y = P.step(y, dtype)
        if trace:
            y64 = y.astype(np.float64)
            lps.append(P.lp64(y64 / y64.sum()))
    y64 = y.astype(np.float64)
    return y64 / y64.sum(), np.array(lps)


def reference_stop_iteration(P, max_iters=5000, eps=1e-6):
    """The iteration at which em.jl itself stops: Float32 iterates, Float32 logs summed into a Float32 (em.jl:71-78), the rule
    lp - lp0 < 1e-6.  Returns (iteration, normalised y)."""
    def lp32(y):
        _, p = P.frag_probs(y, np.float32)
        return np.float32((P.ks.astype(np.float32) * np.log(p)).sum(dtype=np.float32))
    y = np.full(P.n, 1.0 / P.n, np.float32)
    lp = lp32(y)
    for t in range(1, max_iters + 1):
        y = P.step(y, np.float32)
        lp0, lp = lp, lp32(y)
        if float(lp) - float(lp0) < eps:
            y64 = y.astype(np.float64)
            return t, y64 / y64.sum()
    raise AssertionError("the reference's rule did not stop within %d iterations" % max_iters)


def expand_rows(lm, ks):
    """The matrix with row i repeated ks_i times, as a Problem."""
    indptr, col, val = rows_of(lm["m"], lm["n"], lm["colptr"], lm["rowval"], lm["nzval"])
    lens = np.diff(indptr)
    rep = np.repeat(np.arange(lm["m"]), ks)
    new_lens = lens[rep]
    new_indptr = np.concatenate([[0], np.cumsum(new_lens)])
    take = np.concatenate([np.arange(indptr[i], indptr[i + 1]) for i in rep]) if rep.size else np.zeros(0, np.int64)
    return Problem(rep.size, lm["n"], new_indptr, col[take], val[take])


def subset_csc(lm, keep):
    """The matrix with only the entries keep[k] != 0 (same m, n), in the HDF5's CSC form."""
    keep = np.asarray(keep, bool)
    cp = np.asarray(lm["colptr"], np.int64) - 1
    colidx = np.repeat(np.arange(lm["n"]), np.diff(cp))[keep]
    ncp = np.zeros(lm["n"] + 1, np.int64)
    np.cumsum(np.bincount(colidx, minlength=lm["n"]), out=ncp[1:])
    return dict(lm, colptr=(ncp + 1).astype(np.uint32), rowval=np.asarray(lm["rowval"])[keep], nzval=np.asarray(lm["nzval"])[keep])


@pytest.fixture(scope="module")
def fixture_problem(lm_fixture):
    return Problem.from_csc(lm_fixture)


@pytest.fixture(scope="module")
def fixture_run(fixture_problem):
    return run_em(fixture_problem, 3000)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def test_one_step_on_single_transcript_fragments_gives_counts():
    cs = np.array([3, 0, 10, 1, 0, 6], np.int64)
    n, m = cs.size, int(cs.sum())
    indptr = np.arange(m + 1)
    col = np.repeat(np.arange(n), cs)
    rng = np.random.default_rng(0)
    P = Problem(m, n, indptr, col, rng.uniform(0.1, 2.0, m).astype(np.float32))
    for dtype, tol in ((np.float64, 1e-15), (np.float32, 1e-6)):
        y, _ = run_em(P, 1, dtype)
        assert np.allclose(y, cs / m, rtol=tol, atol=0)
        assert (y[cs == 0] == 0).all()


def test_two_transcripts_match_a_brute_force_grid():
    rng = np.random.default_rng(4)
    m = 400
    Xd = rng.uniform(0.05, 1.0, size=(m, 2)).astype(np.float32)
    Xd[np.arange(m), (rng.uniform(size=m) < 0.7).astype(int)] *= np.float32(5)  # (an interior maximum, near 0.3 : 0.7)
    P = Problem(m, 2, np.arange(0, 2 * m + 1, 2), np.tile([0, 1], m), Xd.ravel())
    y, lps = run_em(P, 2000)
    t = np.linspace(0, 1, 200001)[1:-1]
    ll = np.log(np.outer(Xd[:, 0].astype(np.float64), t) + np.outer(Xd[:, 1].astype(np.float64), 1 - t)).sum(axis=0)
    k = int(np.argmax(ll))
    assert 0.1 < t[k] < 0.9 and abs(y[0] - t[k]) <= 2 * (t[1] - t[0])
    assert lps[-1] >= ll[k] - 1e-9 and lps[-1] <= ll[k] + 1e-6


def test_fixture_reaches_the_surveyed_maximum(fixture_problem, fixture_run):
    P = fixture_problem
    assert (P.m, P.n, P.keep.size, P.col.size) == (19743, 313, 19743, 42775)
    u = np.full(P.n, 1.0 / P.n)
    assert abs(P.lp64(u) - -364724.375) < 1e-2
    y, lps = fixture_run
    for t, want, tol in ((1, -328114.515, 1e-2), (100, -326995.495, 1e-2), (200, -326994.548, 1e-2), (1000, -326994.3916, 1e-3)):
        assert abs(lps[t - 1] - want) < tol, (t, lps[t - 1])
    assert abs(lps[-1] - FIXTURE_MAX) < 1e-3, lps[-1]
    assert abs(y.sum() - 1) < 1e-12 and (y >= 0).all()


def test_every_increase_is_non_negative(fixture_problem, fixture_run):
    _, lps = fixture_run
    inc = np.diff(np.concatenate([[fixture_problem.lp64(np.full(313, 1.0 / 313))], lps]))
    assert (inc >= 0).all(), inc.min()
    assert inc[:100].min() > 0.02  # (0.026: the monotonicity test on the device rests on it)
    assert inc[-1] < 1e-8


def test_f32_restatement_stays_close_in_log_likelihood(fixture_problem, fixture_run):
    _, lps64 = fixture_run
    _, lps32 = run_em(fixture_problem, 2000, np.float32)
    assert np.abs(lps32 - lps64[:2000]).max() < 1.5e-4


def test_reference_rule_stops_early_on_the_fixture(fixture_problem):
    t, y = reference_stop_iteration(fixture_problem)
    assert 60 <= t <= 140, t  # (85 here; which increase a Float32 sum first fails to represent depends on the summation order)
    assert FIXTURE_MAX - fixture_problem.lp64(y) > 0.5


def test_multiplicities_equal_the_row_expanded_matrix(lm_fixture):
    rng = np.random.default_rng(7)
    ks = rng.integers(1, 5, lm_fixture["m"])
    Pk = Problem.from_csc(lm_fixture, ks=ks)
    Px = expand_rows(lm_fixture, ks)
    assert Pk.M == Px.M == ks.sum()
    yk, lk = run_em(Pk, 50)
    yx, lx = run_em(Px, 50)
    assert np.abs(yk - yx).max() <= 1e-12
    assert np.abs(lk - lx).max() <= 1e-12 * abs(lk[-1])


def test_empty_rows_are_dropped():
    indptr = np.array([0, 2, 2, 3, 3])
    P = Problem(4, 3, indptr, np.array([0, 2, 2]), np.array([0.5, 0.25, 1.0], np.float32))
    assert P.M == 2
    y, lps = run_em(P, 200)
    assert np.isfinite(lps).all() and y[1] == 0 and abs(y.sum() - 1) < 1e-12


# ---- CSV writer and CLI ---------------------------------------------------------------------------------------------------------
def test_csv_writer_format(tmp_path):
    out = str(tmp_path / "em.csv")
    E.write_csv(out, ["a", "b", "c", "d"], np.array([12.5, 0.0, 1.5e-7, 999999.9], np.float32))
    lines = open(out).read().splitlines()
    assert lines[0] == "transcript_id,tpm"
    assert lines[1:] == ["a,12.5", "b,0.0", "c,1.5e-7", "d,999999.9"]
    for line, v in zip(lines[1:], [12.5, 0.0, 1.5e-7, 999999.9]):
        assert np.float32(float(line.split(",")[1])) == np.float32(v)
    with pytest.raises(ValueError, match="different number of transcripts"):
        E.write_csv(out, ["a"], np.zeros(2, np.float32))
    tr = str(tmp_path / "trace.csv")
    E.write_trace_csv(tr, [-3.5, -3.25])
    assert open(tr).read().splitlines() == ["iteration,lp", "1,-3.5", "2,-3.25"]


def test_cli_rejects_bad_arguments(tmp_path, capsys):
    lm = os.path.join(GOLDEN, "mBr_M_6w_1.likelihood-matrix.h5")
    ids = tmp_path / "ids.txt"
    ids.write_text("\n".join("t%d" % j for j in range(312)) + "\n")
    for argv, msg in (([lm, "--transcript-ids", str(ids)], "312 ids for 313 transcripts"),
                      ([lm, "--max-iters", "0"], "max_iters must be at least 1"),
                      ([lm, "--check-every", "0"], "check_every must be at least 1")):
        with pytest.raises(SystemExit) as e:
            E.main(argv + ["-o", str(tmp_path / "never.csv")])
        assert e.value.code == 2
        assert msg in capsys.readouterr().err
    assert not (tmp_path / "never.csv").exists()
    with pytest.raises(ValueError, match="max_iters"):
        E.expectation_maximization(lm, max_iters=0)
    with pytest.raises(ValueError, match="check_every"):
        E.expectation_maximization(lm, check_every=0)


def test_package_exports_the_em_entry_points():
    import polee_amd
    assert polee_amd.EM is E.EM and polee_amd.expectation_maximization is E.expectation_maximization
