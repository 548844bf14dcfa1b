"""Training of the fragment bias model (polee_bias_train_*, include/polee_hip.h): the reference's
`BiasModel(ts, fraglen_pmf, foreground, background)` (src/bias.jl:677-785) from training fragments, on the GPU or (`host=True`) on
the host threads, and the fragment length model that goes with it (src/fragmodel.jl:263-293, :342-343).

    python -m polee_amd.bias fragments.npz -o bias-model.npz [--seed N] [--device D] [--host]
    python -m polee_amd.bias --reference-dump bias-foreground.csv bias-background.csv -o bias-model.npz

fragments.npz: tseq_ptr i64 [n+1], tseq u8 (0 A, 1 C, 2 G, 3 T, 4 other), transcript i32 (0-based), tpos i64 (1-based, transcript
orientation), fraglen i32; optional bg_transcript / bg_tpos / bg_fraglen (else the background is drawn), optional fraglens (the
OBSERVED fragment lengths, paired-end only, fragmodel.jl:237-239; default: fraglen).  bias-model.npz holds everything
`build_likelihood_matrix(bias=...)` reads, plus fraglen_pmf / fraglen_cdf / fraglen_median.
"""
import argparse
import ctypes as C
import sys

import numpy as np

from . import _lib as L
from ._lib import check, ptr, arr

SEQBIAS_LEN, PS_CTX, GC_EXPANDED, MAX_ROUNDS = 20, 4096, 100, 140
MAX_FRAG_LEN, MIN_FRAG_LEN_COUNT, FALLBACK_FRAGLEN_MEAN, FALLBACK_FRAGLEN_SD, BIAS_EFFLEN_NUM_FRAGLENS = 2000, 1000, 150, 50, 200


class BiasTrainer(L.Handle):
    """A polee_bias_train handle: examples made (create), not yet trained."""
    _destroy = "polee_bias_train_destroy"

    def __init__(self, h, ctx, host):
        self._h, self.ctx, self.host = h, ctx, host

    def _c(self):
        return None if self.host else self.ctx._h

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def run(self):
        check(L.lib().polee_bias_train_run(self._h), self._c())
        return self

    def sizes(self):
        a, b = C.c_int64(), C.c_int64()
        check(L.lib().polee_bias_train_get_examples(self._h, C.byref(a), C.byref(b), None, None, None, None), self._c())
        return a.value, b.value

    def examples(self, positions=True):
        """dict(n_fg, n_bg, left u64 [N], right u64 [N] (20 two-bit codes, position 1 highest), frag_gc f64 [N], bg_tpos i64 [n_bg])"""
        n_fg, n_bg = self.sizes()
        N = n_fg + n_bg
        out = dict(n_fg=n_fg, n_bg=n_bg, left=np.empty(N, np.uint64), right=np.empty(N, np.uint64), frag_gc=np.empty(N, np.float64))
        if positions:
            out["bg_tpos"] = np.empty(n_bg, np.int64)
        check(L.lib().polee_bias_train_get_examples(self._h, None, None, ptr(out["left"], L.u64p), ptr(out["right"], L.u64p),
                                                    ptr(out["frag_gc"], L.f64p), ptr(out.get("bg_tpos"), L.i64p)), self._c())
        return out

    def model(self):
        out = dict(orders_left=np.empty(SEQBIAS_LEN, np.int32), orders_right=np.empty(SEQBIAS_LEN, np.int32),
                   ps_left=np.empty((SEQBIAS_LEN, 4, PS_CTX), np.float32), ps_right=np.empty((SEQBIAS_LEN, 4, PS_CTX), np.float32),
                   gc_bins=np.empty(GC_EXPANDED, np.float32))
        qs, acc = np.empty(14, np.float32), C.c_double()
        check(L.lib().polee_bias_train_get_model(self._h, ptr(out["orders_left"], L.i32p), ptr(out["orders_right"], L.i32p),
                                                 ptr(out["ps_left"], L.f32p), ptr(out["ps_right"], L.f32p), ptr(out["gc_bins"], L.f32p),
                                                 ptr(qs, L.f32p), C.byref(acc)), self._c())
        out["accuracy"] = acc.value
        out["loss_trace_left"], self.positions_left = self.trace(0)
        out["loss_trace_right"], self.positions_right = self.trace(1)
        self.gc_qs = qs
        return out

    def trace(self, side):
        r, pos, loss = C.c_int32(), np.empty(MAX_ROUNDS, np.int32), np.empty(MAX_ROUNDS + 1, np.float64)
        check(L.lib().polee_bias_train_get_trace(self._h, side, C.byref(r), ptr(pos, L.i32p), ptr(loss, L.f64p)), self._c())
        return loss[:r.value + 1].copy(), pos[:r.value].copy()

    def candidates(self, side, orders):
        """(losses f64 [20], loss0) of ONE round from the state `orders` (polee_bias_train_candidates)"""
        o = arr(orders, np.int32)
        assert o.shape == (SEQBIAS_LEN,)
        losses, loss0 = np.empty(SEQBIAS_LEN, np.float64), C.c_double()
        check(L.lib().polee_bias_train_candidates(self._h, side, ptr(o, L.i32p), ptr(losses, L.f64p), C.byref(loss0)), self._c())
        return losses, loss0.value


def _open(host, ctx):
    if host:
        return None
    from .core import default_context
    return ctx or default_context()


def valid_fragments(tseq_ptr, transcript, tpos, fraglen):
    """the fragments BiasedFragModel keeps (fragmodel.jl:227-234): fraglen >= 20, inside their transcript"""
    tseq_ptr = np.asarray(tseq_ptr, np.int64)
    t, p, f = np.asarray(transcript, np.int64), np.asarray(tpos, np.int64), np.asarray(fraglen, np.int64)
    inside = (t >= 0) & (t < len(tseq_ptr) - 1)
    tlen = np.diff(tseq_ptr)[np.where(inside, t, 0)]
    return inside & (f >= SEQBIAS_LEN) & (p >= 1) & (p + f - 1 <= tlen)


def bias_trainer(tseq_ptr, tseq, transcript, tpos, fraglen, background=None, seed=0, host=False, ctx=None):
    """-> (BiasTrainer, dropped): the examples of the fragments that pass valid_fragments; background: (transcript, tpos, fraglen)
    or None = one drawn per kept foreground fragment"""
    ctx = _open(host, ctx)
    tseq_ptr, tseq = arr(tseq_ptr, np.int64), arr(tseq, np.uint8)
    keep = valid_fragments(tseq_ptr, transcript, tpos, fraglen)
    dropped = int((~keep).sum())
    ft, fp, ff = arr(np.asarray(transcript)[keep], np.int32), arr(np.asarray(tpos)[keep], np.int64), arr(np.asarray(fraglen)[keep], np.int32)
    bt = bp = bf = None
    n_bg = len(ft)
    if background is not None:
        kb = valid_fragments(tseq_ptr, *background)
        dropped += int((~kb).sum())
        bt, bp, bf = (arr(np.asarray(a)[kb], dt) for a, dt in zip(background, (np.int32, np.int64, np.int32)))
        n_bg = len(bt)
    opts = L.BiasTrainOpts(int(seed) & (2**64 - 1), int(bool(host)), 0)
    h = C.c_void_p()
    c = None if host else ctx._h
    check(L.lib().polee_bias_train_create(c, len(tseq_ptr) - 1, ptr(tseq_ptr, L.i64p), ptr(tseq, L.u8p), len(ft), ptr(ft, L.i32p),
                                          ptr(fp, L.i64p), ptr(ff, L.i32p), n_bg, ptr(bt, L.i32p), ptr(bp, L.i64p), ptr(bf, L.i32p),
                                          C.byref(opts), C.byref(h)), c)
    return BiasTrainer(h, ctx, host), dropped


def examples_trainer(left_seq, right_seq, frag_gc, n_fg, seed=0, host=False, ctx=None):
    """BiasTrainer on ready-made examples: left_seq / right_seq u8 [N, 20] codes, frag_gc f64 [N], the first n_fg foreground"""
    ctx = _open(host, ctx)
    l, r, g = arr(left_seq, np.uint8), arr(right_seq, np.uint8), arr(frag_gc, np.float64)
    assert l.ndim == 2 and l.shape[1] == SEQBIAS_LEN and l.shape == r.shape and g.shape == (l.shape[0],)
    opts = L.BiasTrainOpts(int(seed) & (2**64 - 1), int(bool(host)), 0)
    h = C.c_void_p()
    c = None if host else ctx._h
    check(L.lib().polee_bias_train_create_from_examples(c, int(n_fg), len(g) - int(n_fg), ptr(l, L.u8p), ptr(r, L.u8p), ptr(g, L.f64p),
                                                        C.byref(opts), C.byref(h)), c)
    return BiasTrainer(h, ctx, host)


def train_bias_model(tseq_ptr, tseq, transcript, tpos, fraglen, background=None, seed=0, host=False, ctx=None):
    """BiasModel(...) (src/bias.jl:677-785) -> dict(orders_left, orders_right i32 [20], ps_left, ps_right f32 [20, 4, 4096], gc_bins f32
    [100] -- the keys xbuild.pack_bias reads for the sequence models and the GC model -- accuracy (a fraction), loss_trace_left /
    loss_trace_right f64 [rounds + 1], dropped: the fragments left out as the reference leaves them out (fragmodel.jl:227-234))."""
    bt, dropped = bias_trainer(tseq_ptr, tseq, transcript, tpos, fraglen, background, seed, host, ctx)
    with bt:
        out = bt.run().model()
    out["dropped"] = dropped
    return out


def train_bias_model_from_examples(left_seq, right_seq, frag_gc, n_fg, seed=0, host=False, ctx=None):
    """the same from ready-made examples (read_reference_dump)"""
    with examples_trainer(left_seq, right_seq, frag_gc, n_fg, seed, host, ctx) as bt:
        out = bt.run().model()
    out["dropped"] = 0
    return out


def bias_training_examples(tseq_ptr, tseq, transcript, tpos, fraglen, background=None, seed=0, host=False, ctx=None):
    """the examples alone (BiasTrainingExample, src/bias.jl:21-80): BiasTrainer.examples() + dropped"""
    bt, dropped = bias_trainer(tseq_ptr, tseq, transcript, tpos, fraglen, background, seed, host, ctx)
    with bt:
        out = bt.examples()
    out["dropped"] = dropped
    return out


def bias_candidate_losses(trainer, side, orders):
    return trainer.candidates(side, orders)


def fragment_length_model(fraglens):
    """The fragment length part of BiasedFragModel (src/fragmodel.jl:263-293, :342-343), host NumPy: dict(fraglen_pmf f32 [2000],
    fraglen_cdf f32 [2000], fraglen_median, high_prob_fraglens i32 [200]).  pmf: pseudocount 1 plus the observed lengths <= 2000, or
    the Normal(150, 50) fallback below 1000 observations; the normalising sum is exact for counts below 2^24 (the fallback's is taken
    in f32 over two halves in sequence -- Julia's own order is its SIMD loop's).  high_prob_fraglens: the 200 most probable lengths in a
    STABLE descending sort (equal probabilities: the shorter length first, as sortperm(rev=true) leaves them)."""
    fl = np.asarray(fraglens, np.int64).ravel()
    hist = np.bincount(fl[(fl >= 1) & (fl <= MAX_FRAG_LEN)] - 1, minlength=MAX_FRAG_LEN)
    return fragment_length_model_from_hist(hist, len(fl))


def fragment_length_model_from_hist(hist, num_observations=None):
    """The same from a histogram: hist[l-1] = observations of length l <= 2000; num_observations: what is held against the 1000 of the
    fallback (fragment_length_model: every length it was given, SimplisticFragModel: those <= 2000 = hist.sum(), the default)."""
    hist = np.asarray(hist, np.int64).ravel()
    assert hist.shape == (MAX_FRAG_LEN,)
    if (int(hist.sum()) if num_observations is None else int(num_observations)) < MIN_FRAG_LEN_COUNT:
        x = np.arange(1, MAX_FRAG_LEN + 1, dtype=np.float64)
        z = (x - FALLBACK_FRAGLEN_MEAN) / FALLBACK_FRAGLEN_SD
        pmf = (np.exp(-(z * z) / 2) * 0.3989422804014326779 / FALLBACK_FRAGLEN_SD).astype(np.float32)
        half = MAX_FRAG_LEN // 2
        total = np.float32(np.cumsum(pmf[:half], dtype=np.float32)[-1] + np.cumsum(pmf[half:], dtype=np.float32)[-1])
    else:
        counts = 1 + hist
        pmf = counts.astype(np.float32)
        total = np.float32(int(counts.sum()))
    pmf = (pmf / total).astype(np.float32)
    cdf = np.cumsum(pmf, dtype=np.float32)
    return dict(fraglen_pmf=pmf, fraglen_cdf=cdf, fraglen_median=int(np.searchsorted(cdf, 0.5, "left")) + 1,
                high_prob_fraglens=(np.argsort(-pmf, kind="stable")[:BIAS_EFFLEN_NUM_FRAGLENS] + 1).astype(np.int32))


_CODE = np.full(256, 4, np.uint8)
for _i, _ch in enumerate("ACGT"):
    _CODE[ord(_ch)] = _CODE[ord(_ch.lower())] = _i


def read_reference_dump(foreground_csv, background_csv):
    """The reference's --dump-bias-training-examples files (src/fragmodel.jl:306-339): one example per line,
    left_seq,right_seq,frag_gc,tpdist,fpdist,tlen,flen,<freqs...>; only the first three fields are used.
    -> (left_seq u8 [N, 20], right_seq u8 [N, 20], frag_gc f64 [N], n_fg)"""
    left, right, gc, n_fg = [], [], [], 0
    for k, path in enumerate((foreground_csv, background_csv)):
        with open(path) as f:
            for lineno, line in enumerate(f, 1):
                line = line.strip()
                if not line:
                    continue
                fields = line.split(",")
                if len(fields) < 3 or len(fields[0]) != SEQBIAS_LEN or len(fields[1]) != SEQBIAS_LEN:
                    raise ValueError("%s:%d: expected two %d-base sequences and frag_gc" % (path, lineno, SEQBIAS_LEN))
                left.append(_CODE[np.frombuffer(fields[0].encode("ascii"), np.uint8)])
                right.append(_CODE[np.frombuffer(fields[1].encode("ascii"), np.uint8)])
                gc.append(float(fields[2]))
                n_fg += k == 0
    return (np.array(left, np.uint8).reshape(-1, SEQBIAS_LEN), np.array(right, np.uint8).reshape(-1, SEQBIAS_LEN),
            np.array(gc, np.float64), n_fg)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m polee_amd.bias", description="train the fragment bias model (src/bias.jl)")
    ap.add_argument("fragments", nargs="?", help="fragments.npz (see the module's docstring)")
    ap.add_argument("-o", "--output", required=True)
    ap.add_argument("--reference-dump", nargs=2, metavar=("FOREGROUND_CSV", "BACKGROUND_CSV"),
                    help="train on the reference's --dump-bias-training-examples files instead of fragments")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--host", action="store_true", help="train on the host threads (POLEE_HOST_THREADS), no GPU")
    a = ap.parse_args(argv)
    if a.fragments is None and a.reference_dump is None:
        ap.error("fragments.npz or --reference-dump is required")
    ctx = None
    if not a.host:
        from .core import Context
        ctx = Context(a.device)
    out = {}
    z = np.load(a.fragments) if a.fragments else None
    if z is not None:
        out.update(tseq_ptr=np.asarray(z["tseq_ptr"], np.int64), tseq=np.asarray(z["tseq"], np.uint8))
    if a.reference_dump:
        l, r, g, n_fg = read_reference_dump(*a.reference_dump)
        model = train_bias_model_from_examples(l, r, g, n_fg, seed=a.seed, host=a.host, ctx=ctx)
        fraglens = z["fraglens"] if z is not None and "fraglens" in z.files else None
    else:
        bg = (z["bg_transcript"], z["bg_tpos"], z["bg_fraglen"]) if "bg_transcript" in z.files else None
        model = train_bias_model(z["tseq_ptr"], z["tseq"], z["transcript"], z["tpos"], z["fraglen"], bg, seed=a.seed, host=a.host, ctx=ctx)
        fraglens = z["fraglens"] if "fraglens" in z.files else z["fraglen"]
    out.update(model)
    if fraglens is not None:
        out.update(fragment_length_model(fraglens))
    np.savez(a.output, **out)
    print("bias model: accuracy %.4f, %d + %d rounds, %d fragments dropped -> %s" % (
        model["accuracy"], len(model["loss_trace_left"]) - 1, len(model["loss_trace_right"]) - 1, model["dropped"], a.output))
    return 0


if __name__ == "__main__":
    sys.exit(main())
