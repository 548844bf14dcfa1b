"""Bitwise A/B of the draw-fed models (classify, tsne, random-forest; csrc/draw_model.hpp) between two builds of the library.

    POLEE_HIP_LIB=<build A> python tools/probe/draw_model_ab.py --out a.txt
    POLEE_HIP_LIB=<build B> python tools/probe/draw_model_ab.py --out b.txt
    python tools/probe/draw_model_ab.py --compare a.txt b.txt

Every case runs the models' entry points on the draw path (fixed seeds, and fixed z0 where the entry takes it) and on the point path
and prints a SHA-256 of the raw bytes of each result.  The shapes sit at the edges of the shared blocks: n = 130 (one ragged chunk,
the second lane slot empty) and 1100 (nine chunks, the last of 76 transcripts), S = 3 and 70 (a second LDS tile of 6 samples), k / C
of 1, 2, 3, 5 and 16 (every KP, with padded columns).  --compare prints the lines that differ and the verdict.
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CLASSIFY = [(130, 3, 2), (1100, 70, 3), (1100, 3, 5), (130, 70, 16)]   # n, S, k
TSNE = [(130, 3, 1, 3), (1100, 70, 2, 70), (1100, 5, 3, 4), (130, 70, 5, 9), (1100, 3, 16, 3)]  # n, S, C, B
FOREST = [(130, 3, 2), (1100, 5, 5)]  # n, S, k


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:24]


def problem(P, ctx, S, n):
    """per-sample parameters on one random tree"""
    from tools import synth
    rng = np.random.default_rng(1000 * S + n)
    li, ri, fi = P.make_inverse_ptt_params(*synth.make_tree(np.zeros(n, np.int32), seed=n, kind="random"))
    return P.RNASeqApproxLikelihood(dict(efflen=rng.uniform(200, 3000, size=(S, n)).astype(np.float32),
                                         la_mu=rng.normal(0, 1, size=(S, n - 1)).astype(np.float32),
                                         la_sigma=np.exp(rng.normal(-1, 0.3, size=(S, n - 1))).astype(np.float32),
                                         la_alpha=rng.normal(0, 0.3, size=(S, n - 1)).astype(np.float32), left_index=li[None],
                                         right_index=ri[None], leaf_index=fi[None]), ctx=ctx)


def points(S, n):
    rng = np.random.default_rng(3000 * S + n)
    return rng.normal(-np.log(n), 1.5, size=(S, n)).astype(np.float32)


def classify_case(P, ctx, emit, n, S, k):
    tag = "classify n=%d S=%d k=%d" % (n, S, k)
    rng = np.random.default_rng(7 * n + S + k)
    ap, x, D = problem(P, ctx, S, n), points(S, n), 2
    y = np.eye(k, dtype=np.float32)[rng.integers(0, k, S)]
    w0 = (rng.normal(0, 0.1, size=(n, k)).astype(np.float32), rng.normal(-7, 1, n).astype(np.float32),
          rng.normal(0, 0.1, k).astype(np.float32))
    z0 = rng.normal(size=(5, D, S, n - 1)).astype(np.float32)
    clf = P.RNASeqLogisticRegression(k, n, ctx=ctx, draws_per_step=D, learning_rate=1e-2)
    clf.init_bias_sample(S, n, ap, seed=11)
    emit(tag, "init_bias_sample", digest(*clf.get_params()))
    clf.set_params(*w0)
    emit(tag, "loss_and_gradients z0", digest(*clf.loss_and_gradients(S, n, ap, y, z0=z0[0])[1:]),
         repr(clf.loss_and_gradients(S, n, ap, y, z0=z0[0])[0]))
    emit(tag, "loss_and_gradients seed", digest(*clf.loss_and_gradients(S, n, ap, y, seed=12)[1:]))
    clf.reset()
    emit(tag, "fit_steps_sample z0 trace", digest(clf.fit_steps_sample(S, n, ap, y, 5, z0=z0)))
    emit(tag, "fit_steps_sample z0 params", digest(*clf.get_params()))
    emit(tag, "fit_steps_sample seed trace", digest(clf.fit_steps_sample(S, n, ap, y, 5, seed=13)))
    emit(tag, "fit_steps_sample seed params", digest(*clf.get_params()))
    emit(tag, "predict_sample z0", digest(clf.predict_sample(S, n, ap, 3, z0=z0[0, 0:1].repeat(3, 0))))
    emit(tag, "predict_sample seed", digest(clf.predict_sample(S, n, ap, 3, seed=14)))
    clf.init_bias(x)
    clf.set_params(w0[0], clf.get_params()[1], w0[2])
    clf.reset()
    emit(tag, "points loss_and_gradients", digest(*clf.loss_and_gradients(x=x, z_true=y)[1:]))
    emit(tag, "points fit_steps trace", digest(clf.fit_steps(x, y, 5)))
    emit(tag, "points fit_steps params", digest(*clf.get_params()))
    emit(tag, "points predict", digest(clf.predict(x)))


def tsne_case(P, ctx, emit, n, S, C, B):
    tag = "tsne n=%d S=%d C=%d B=%d" % (n, S, C, B)
    rng = np.random.default_rng(5 * n + S + C)
    ap, x = problem(P, ctx, S, n), points(S, n)
    W0 = rng.normal(0, 0.1, size=(n, C)).astype(np.float32)
    z0 = rng.normal(size=(5, S, n - 1)).astype(np.float32)
    batches = np.array([rng.permutation(S)[:B] for _ in range(5)], np.int32)
    for path, src in (("draws", dict(vars=ap)), ("points", dict(x=x))):
        ts = P.RNASeqTSNE(n, S, ctx=ctx, num_components=C, learning_rate=1e-3)
        zkw = dict(z0=z0[0]) if path == "draws" else {}
        delta = ts.distances(**src, **zkw)
        emit(tag, path + " distances", digest(delta))
        if path == "draws":
            emit(tag, path + " distances seed", digest(ts.distances(ap, seed=21)))
        ts.set_sigmas(np.sqrt(np.median(delta[delta > 0])) * np.linspace(0.5, 1.5, S))
        ts.set_params(W0)
        loss, gw = ts.loss_and_gradient(batches[0], **src, **zkw)
        emit(tag, path + " loss_and_gradient", digest(gw), repr(loss))
        emit(tag, path + " fit trace", digest(ts.fit(5, batches=batches, **src, **(dict(z0=z0) if path == "draws" else {}))))
        emit(tag, path + " fit W", digest(ts.get_params()))
        if path == "draws":
            emit(tag, path + " fit seed trace", digest(ts.fit(5, batches=batches, vars=ap, seed=22)))
            emit(tag, path + " fit seed W", digest(ts.get_params()))
            emit(tag, path + " embed z0", digest(ts.embed(ap, ndraws=3, z0=z0[:3])))
            emit(tag, path + " embed seed", digest(ts.embed(ap, ndraws=3, seed=23)))
        else:
            emit(tag, path + " embed", digest(ts.embed(x=x)))


def forest_case(P, ctx, emit, n, S, k):
    from polee_amd.random_forest import RNASeqRandomForest, log_draws
    tag = "forest n=%d S=%d k=%d" % (n, S, k)
    rng = np.random.default_rng(3 * n + S + k)
    ap, D = problem(P, ctx, S, n), 4
    y = (np.arange(S) % k).astype(np.int32)
    z0 = rng.normal(size=(D, S, n - 1)).astype(np.float32)
    emit(tag, "log_draws z0", digest(log_draws(ap, D, z0=z0)))
    emit(tag, "log_draws seed", digest(log_draws(ap, D, seed=31)))
    for how, kw in (("z0", dict(z0=z0)), ("seed", dict(draw_seed=32))):
        f = RNASeqRandomForest(k, n, ctx=ctx, ntrees=8).fit_sample(ap, y, D, seed=33, **kw)
        emit(tag, "fit_sample %s nodes" % how, digest(*f.nodes()))
        emit(tag, "votes_sample %s" % how, digest(f.votes_sample(ap, D, **(dict(z0=z0) if how == "z0" else dict(seed=34)))))
    x = points(S * D, n)
    f = RNASeqRandomForest(k, n, ctx=ctx, ntrees=8).fit(x, np.tile(y, D), seed=35)
    emit(tag, "points fit nodes", digest(*f.nodes()))
    emit(tag, "points votes", digest(f.votes(x)))


def compare(a, b):
    la, lb = (open(p).read().splitlines() for p in (a, b))
    ra, rb = ([l for l in ls if not l.startswith("build:")] for ls in (la, lb))
    bad = [(x, y) for x, y in zip(ra, rb) if x != y]
    for x, y in bad:
        print("DIFFERS\n  %s\n  %s" % (x, y))
    ok = not bad and len(ra) == len(rb) and len(ra) > 0
    print("verdict: %d results, %s" % (len(ra), "every hash equal" if ok else "%d differ (or the files are of unequal length)" % len(bad)))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    import polee_amd as P
    ctx = P.Context(0)
    lines = ["build: " + P.version(), "build: library " + os.path.relpath(P._lib.LIB_PATH, ROOT)]

    def emit(tag, what, *vals):
        lines.append("%-28s %-30s %s" % (tag, what, " ".join(vals)))
        print(lines[-1], flush=True)

    print("\n".join(lines), flush=True)
    for case in CLASSIFY:
        classify_case(P, ctx, emit, *case)
    for case in TSNE:
        tsne_case(P, ctx, emit, *case)
    for case in FOREST:
        forest_case(P, ctx, emit, *case)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
