"""The fragment model from the alignment pairs themselves (polee_fragmodel_estimate, polee_read_assign, include/polee_hip.h; DESIGN.md
section 3.18): what the reference does between reading the alignments and building X (src/rnaseq_sample.jl:330-380) -- subsample the
reads, SimplisticFragModel from the subset (src/fragmodel.jl:35-113), X of the subset under it, the mixture, one transcript per read,
BiasedFragModel's length model and strand specificity from the assigned reads (src/fragmodel.jl:186-293) and the bias model.

    python -m polee_amd.fragmodel alignments.npz -o fragment-model.npz [--no-bias] [--num-training-reads N] [--alt-frag-model]
                                  [--seed N] [--assign draw|reference] [--mixture optimize|em] [--device D]

alignments.npz holds the arrays of polee_xb_transcripts and polee_xb_fragments under their field names -- exon_ptr, exon_first, exon_last;
seq, strand, m1_left, m1_right, m2_left, m2_right, m1_is_flag16, cig1_ptr, cig2_ptr, cig_op, cig_len -- with the transcripts' own seq and
strand, which would collide with the fragments', as t_seq and t_strand; plus tseq_ptr i64 [n+1], tseq u8 (0 A, 1 C, 2 G, 3 T, 4 other) and
optionally m1_reverse u8 [m].  A fragment is one alignment pair of one read (there are no read ids: one pair is one read).
fragment-model.npz: save_model / load_model.  There is no --host: the two kernels have no host twin.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

from . import _lib as L
from . import bias as B
from . import xbuild as XB
from ._lib import check, ptr, arr

MAX_FRAG_LEN, FALLBACK_FRAGLEN_MEAN, NUM_TRAINING_READS = B.MAX_FRAG_LEN, B.FALLBACK_FRAGLEN_MEAN, 200000
FLAG_OBSERVED, FLAG_STRAND_MATCH, FLAG_STRAND_MISMATCH = 1, 2, 4
ASSIGN_MODES = {"draw": 0, "reference": 1}
NO_OVERLAP = ("No reads overlap any transcripts. This is usally because a set of transcripts was provided that doesn't match "
              "transcriptome or genome that the reads were aligned to.")  # (the reference's words, fragmodel.jl:71-75)
_F_PER_FRAGMENT = ("seq", "strand", "m1_left", "m1_right", "m2_left", "m2_right", "m1_is_flag16")


def _ctx(ctx):
    from .core import default_context
    return ctx or default_context()


def subsample_fragments(fragments, num_training_reads=NUM_TRAINING_READS, seed=0):
    """-> (subset, indices).  The reference keeps a reservoir of reads with distinct start positions (subsample_reads, src/reads.jl:386-438:
    its stream of random numbers is Julia's).  Here, reproducible from the seed: the distinct (seq, m1_left) keys after order_mates,
    min(num_training_reads, #keys) of them chosen without replacement by np.random.Generator(np.random.Philox(key=seed)) from the keys
    in ascending order, and for every chosen key its lowest-index fragment.  subset: those fragments, in input order, in the layout of
    polee_xb_fragments with their CIGAR ranges repacked; indices i64: where they were."""
    F = XB.order_mates(fragments)
    m = int(F["m"])
    keys = np.stack([np.asarray(F["seq"], np.int64)[:m], np.asarray(F["m1_left"], np.int64)[:m]], axis=1)
    _, first = np.unique(keys, axis=0, return_index=True)
    size = min(int(num_training_reads), len(first))
    if size < 0:
        raise ValueError("num_training_reads must not be negative")
    if size < len(first):
        rng = np.random.Generator(np.random.Philox(key=int(seed) & (2 ** 64 - 1)))
        first = first[rng.choice(len(first), size=size, replace=False)]
    idx = np.sort(first).astype(np.int64)
    return take_fragments(F, idx), idx


def take_fragments(fragments, idx):
    """the fragments idx of a polee_xb_fragments dict (mates ordered), CIGAR ranges repacked"""
    F = XB.order_mates(fragments)
    idx = np.asarray(idx, np.int64)
    out = dict(m=len(idx))
    for k in _F_PER_FRAGMENT:
        out[k] = np.ascontiguousarray(np.asarray(F[k])[idx])
    c1, c2 = np.asarray(F["cig1_ptr"], np.int64), np.asarray(F["cig2_ptr"], np.int64)
    n1, n2 = (c1[1:] - c1[:-1])[idx], (c2[1:] - c2[:-1])[idx]
    p1 = np.concatenate([[0], np.cumsum(n1)]).astype(np.int64)
    p2 = (p1[-1] + np.concatenate([[0], np.cumsum(n2)])).astype(np.int64)  # (all first mates' operations, then all second mates')
    src = np.concatenate([np.repeat(c1[:-1][idx] - p1[:-1], n1) + np.arange(p1[-1]),
                          np.repeat(c2[:-1][idx] - p2[:-1], n2) + np.arange(p1[-1], p2[-1])]).astype(np.int64)
    out["cig_op"] = np.asarray(F["cig_op"], np.uint8)[src] if src.size else np.zeros(1, np.uint8)
    out["cig_len"] = np.asarray(F["cig_len"], np.int32)[src] if src.size else np.zeros(1, np.int32)
    out["cig1_ptr"], out["cig2_ptr"] = p1, p2
    return out


def simplistic_from_counts(counts, hist, alt_frag_model=False):
    """SimplisticFragModel's fields (src/fragmodel.jl:69-112) from polee_fragmodel_estimate's integers, host NumPy"""
    match, mismatch = int(counts[1]), int(counts[2])
    if match + mismatch == 0:
        raise ValueError(NO_OVERLAP)
    lm = B.fragment_length_model_from_hist(hist)
    return dict(fraglen_pmf=lm["fraglen_pmf"], fraglen_cdf=lm["fraglen_cdf"], fraglen_median=lm["fraglen_median"],
                strand_specificity=float(np.float32(match / (match + mismatch))), alt_frag_model=bool(alt_frag_model))


def fragmodel_counts(transcripts, fragments, ctx=None, return_min_fraglen=True):
    """polee_fragmodel_estimate -> dict(counts i64 [4] = compatible pairs, strand matches, strand mismatches, fragments whose
    length is above 2000; hist i64 [2000]; min_fraglen i64 [m], 0 = none)"""
    ctx = _ctx(ctx)
    F = XB.order_mates(fragments)
    T, Fs, keep = XB.pack_tf(transcripts, F)
    out = dict(counts=np.zeros(4, np.int64), hist=np.zeros(MAX_FRAG_LEN, np.int64))
    if return_min_fraglen:
        out["min_fraglen"] = np.zeros(int(F["m"]), np.int64)
    check(L.lib().polee_fragmodel_estimate(ctx._h, C.byref(T), C.byref(Fs), ptr(out["counts"], L.i64p), ptr(out["hist"], L.i64p),
                                           ptr(out.get("min_fraglen"), L.i64p)), ctx._h)
    del keep
    return out


def estimate_simplistic(transcripts, fragments, alt_frag_model=False, ctx=None):
    """SimplisticFragModel(rs, ts, alt_frag_model) (src/fragmodel.jl:35-113) -> dict(fraglen_pmf, fraglen_cdf f32 [2000], fraglen_median,
    strand_specificity, alt_frag_model -- the five build_likelihood_matrix takes -- and counts = dict(compatible_pairs, strand_match,
    strand_mismatch, long_fragments, fragments_with_length)).  The counts are made on the GPU, the rest is host NumPy."""
    c = fragmodel_counts(transcripts, fragments, ctx, return_min_fraglen=False)
    out = simplistic_from_counts(c["counts"], c["hist"], alt_frag_model)
    out["counts"] = dict(compatible_pairs=int(c["counts"][0]), strand_match=int(c["counts"][1]), strand_mismatch=int(c["counts"][2]),
                         long_fragments=int(c["counts"][3]), fragments_with_length=int(c["hist"].sum()) + int(c["counts"][3]))
    return out


def assign_reads(xbuild, transcripts, fragments, tseq_ptr, xs=None, m1_reverse=None, seed=0, assign="draw",
                 fallback_fraglen=FALLBACK_FRAGLEN_MEAN, ctx=None):
    """polee_read_assign: one transcript per row of `xbuild` (xbuild.XBuild: build_likelihood_matrix(return_xbuild=True) on the same
    transcripts and fragments) and the fragment's interval on it -> dict(transcript i32 (0-based), tpos i64, fraglen i32, flags u8,
    all [rows]).  assign "draw": in proportion to xs[j] X[i, j]; "reference": the last entry of every row, which is what the
    reference's loop does as it is written (xs and seed are not used)."""
    if assign not in ASSIGN_MODES:
        raise ValueError("assign must be one of %s" % sorted(ASSIGN_MODES))
    ctx = _ctx(ctx)
    F = XB.order_mates(fragments)
    T, Fs, keep = XB.pack_tf(transcripts, F)
    n = int(transcripts["n"])
    tp = arr(tseq_ptr, np.int64)
    if tp.shape != (n + 1,):
        raise ValueError("tseq_ptr: %s given for %d transcripts" % (tp.shape, n))
    x = None
    if assign == "draw":
        x = arr(xs, np.float32)
        if x.shape != (n,):
            raise ValueError("xs: %s given for %d transcripts" % (x.shape, n))
    rev = None if m1_reverse is None else arr(m1_reverse, np.uint8)
    if rev is not None and rev.shape != (int(F["m"]),):
        raise ValueError("m1_reverse: %s given for %d fragments" % (rev.shape, int(F["m"])))
    rows, nnz = C.c_int64(), C.c_int64()
    check(L.lib().polee_xbuild_sizes(xbuild._h, C.byref(rows), C.byref(nnz), None, None, None), ctx._h)
    r = rows.value
    out = dict(transcript=np.zeros(r, np.int32), tpos=np.zeros(r, np.int64), fraglen=np.zeros(r, np.int32), flags=np.zeros(r, np.uint8))
    check(L.lib().polee_read_assign(ctx._h, xbuild._h, C.byref(T), C.byref(Fs), ptr(tp, L.i64p), ptr(rev, L.u8p), ptr(x, L.f32p),
                                    C.c_uint64(int(seed) & (2 ** 64 - 1)), ASSIGN_MODES[assign], int(fallback_fraglen),
                                    ptr(out["transcript"], L.i32p), ptr(out["tpos"], L.i64p), ptr(out["fraglen"], L.i32p),
                                    ptr(out["flags"], L.u8p)), ctx._h)
    del keep
    return out


def biased_from_assignment(tseq_ptr, assignment, alt_frag_model=False):
    """BiasedFragModel's length model and strand specificity (src/fragmodel.jl:221-293) from assign_reads' arrays, host NumPy: the five
    fields of a fragment model plus high_prob_fraglens"""
    flags = assignment["flags"]
    match, mismatch = int(((flags & FLAG_STRAND_MATCH) != 0).sum()), int(((flags & FLAG_STRAND_MISMATCH) != 0).sum())
    if match + mismatch == 0:
        raise ValueError(NO_OVERLAP)
    valid = B.valid_fragments(tseq_ptr, assignment["transcript"], assignment["tpos"], assignment["fraglen"])
    lm = B.fragment_length_model(assignment["fraglen"][valid & ((flags & FLAG_OBSERVED) != 0)])
    lm.update(strand_specificity=float(np.float32(match / (match + mismatch))), alt_frag_model=bool(alt_frag_model))
    return lm


def train_fragment_model(transcripts, fragments, tseq_ptr, tseq, m1_reverse=None, no_bias=False, num_training_reads=NUM_TRAINING_READS,
                         alt_frag_model=False, seed=0, assign="draw", mixture="optimize", ctx=None):
    """The reference's training of the fragment model (src/rnaseq_sample.jl:330-380) -> dict(fragmodel, bias, diagnostics).
    fragmodel: the SimplisticFragModel of the training subset (estimate_simplistic).  bias (None with no_bias): the trained bias model
    with tseq_ptr, tseq, high_prob_fraglens and m1_reverse -- the `bias=` argument of build_likelihood_matrix on the FULL fragments
    -- and BiasedFragModel's own fraglen_pmf, fraglen_cdf, fraglen_median, strand_specificity, alt_frag_model, which are that call's
    other arguments.  diagnostics: indices (the subset), counts, rows, nnz, xs, row_fragment, transcript, tpos, fraglen, flags,
    seconds per phase.  mixture "optimize": optimize_likelihood over list_nodes(n), as the reference does; "em": em.EM."""
    if assign not in ASSIGN_MODES:
        raise ValueError("assign must be one of %s" % sorted(ASSIGN_MODES))
    if mixture not in ("optimize", "em"):
        raise ValueError("mixture must be 'optimize' or 'em'")
    ctx = _ctx(ctx)
    n = int(transcripts["n"])
    phases = []
    t0 = [time.perf_counter()]

    def phase(name):
        t = time.perf_counter()
        phases.append((name, t - t0[0]))
        t0[0] = t
    rev = None if m1_reverse is None else arr(m1_reverse, np.uint8)
    sub, idx = subsample_fragments(fragments, num_training_reads, seed)
    rev_sub = None if rev is None else np.ascontiguousarray(rev[idx])
    phase("subsample")
    fm = estimate_simplistic(transcripts, sub, alt_frag_model, ctx)
    phase("estimate")
    diag = dict(indices=idx, counts=fm["counts"])
    out = dict(fragmodel={k: fm[k] for k in ("fraglen_pmf", "fraglen_cdf", "fraglen_median", "strand_specificity", "alt_frag_model")},
               bias=None, diagnostics=diag)
    if not no_bias:
        x = XB.build_likelihood_matrix(transcripts, sub, fm["fraglen_pmf"], fm["fraglen_cdf"], fm["fraglen_median"], fm["strand_specificity"],
                                       alt_frag_model, ctx=ctx, return_sample=True, return_xbuild=True)
        phase("likelihood matrix")
        try:
            if mixture == "optimize":
                from .core import PolyaTreeTransform, list_nodes, optimize_likelihood
                xs = optimize_likelihood(x["sample"], PolyaTreeTransform(*list_nodes(n), ctx=ctx))["x"]
            else:
                from .em import EM
                with_em = EM(x["sample"])
                try:
                    with_em.run()
                    xs = with_em.mixture()
                finally:
                    with_em.close()
            phase("mixture")
            a = assign_reads(x["xbuild"], transcripts, sub, tseq_ptr, xs, rev_sub, seed, assign, ctx=ctx)
            phase("assign")
        finally:
            x["xbuild"].close()
            x["sample"].close()
        lm = biased_from_assignment(tseq_ptr, a, alt_frag_model)
        phase("length model")
        model = B.train_bias_model(tseq_ptr, tseq, a["transcript"], a["tpos"], a["fraglen"], seed=seed, ctx=ctx)
        phase("bias model")
        model.update(lm)
        model.update(tseq_ptr=arr(tseq_ptr, np.int64), tseq=arr(tseq, np.uint8))
        if rev is not None:
            model["m1_reverse"] = rev
        out["bias"] = model
        diag.update(rows=x["m"], nnz=x["nnz"], xs=xs, row_fragment=x["row_fragment"], **a)
    diag["seconds"] = dict(phases)
    if os.environ.get("POLEE_BUILD_TIMING") == "1":
        for name, s in phases:
            sys.stderr.write("train_fragment_model: %-18s %9.3f s\n" % (name, s))
    return out


# ---- files ---------------------------------------------------------------------------------------------------------------------
_SEP = "__"


def save_model(path, model):
    """train_fragment_model's dict as one npz: fragmodel__<field>, bias__<field>, diagnostics__<field> (arrays and numbers)"""
    flat = {}
    for part in ("fragmodel", "bias", "diagnostics"):
        for k, v in (model.get(part) or {}).items():
            if isinstance(v, dict):
                for k2, v2 in v.items():
                    flat[part + _SEP + k + _SEP + k2] = np.asarray(v2)
            else:
                flat[part + _SEP + k] = np.asarray(v)
    flat["has_bias"] = np.asarray(model.get("bias") is not None)
    np.savez(path, **flat)


def load_model(path):
    z = np.load(path)
    out = dict(fragmodel={}, bias={} if bool(z["has_bias"]) else None, diagnostics={})
    for key in z.files:
        parts = key.split(_SEP)
        if len(parts) < 2 or out.get(parts[0]) is None:
            continue
        v = z[key]
        v = v.item() if v.ndim == 0 else v
        if len(parts) == 2:
            out[parts[0]][parts[1]] = v
        else:
            out[parts[0]].setdefault(parts[1], {})[parts[2]] = v
    return out


def read_alignments(path):
    """alignments.npz (the module's docstring) -> (transcripts, fragments, tseq_ptr, tseq, m1_reverse or None)"""
    z = np.load(path)
    need = ["t_seq", "t_strand", "exon_ptr", "exon_first", "exon_last", "tseq_ptr", "tseq"] + list(XB._F_TYPES)
    missing = [k for k in need if k not in z.files]
    if missing:
        raise ValueError("%s: missing %s" % (path, ", ".join(missing)))
    T = dict(n=len(z["t_seq"]), seq=z["t_seq"], strand=z["t_strand"], exon_ptr=z["exon_ptr"], exon_first=z["exon_first"],
             exon_last=z["exon_last"])
    F = {k: z[k] for k in XB._F_TYPES}
    F["m"] = len(F["seq"])
    return T, F, z["tseq_ptr"], z["tseq"], (z["m1_reverse"] if "m1_reverse" in z.files else None)


def parser():
    ap = argparse.ArgumentParser(prog="python -m polee_amd.fragmodel",
                                 description="train the fragment model from alignment pairs (src/rnaseq_sample.jl:330-380)")
    ap.add_argument("alignments", help="alignments.npz (see the module's docstring)")
    ap.add_argument("-o", "--output", required=True)
    ap.add_argument("--no-bias", action="store_true", help="stop at the SimplisticFragModel")
    ap.add_argument("--num-training-reads", type=int, default=NUM_TRAINING_READS)
    ap.add_argument("--alt-frag-model", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--assign", choices=sorted(ASSIGN_MODES), default="draw",
                    help="draw: in proportion to the mixture; reference: the last compatible transcript, as the reference is written")
    ap.add_argument("--mixture", choices=("optimize", "em"), default="optimize")
    ap.add_argument("--device", type=int, default=0)
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    if a.num_training_reads < 1:
        ap.error("--num-training-reads must be at least 1")
    if a.device < 0:
        ap.error("--device must not be negative")
    T, F, tseq_ptr, tseq, rev = read_alignments(a.alignments)
    from .core import Context
    ctx = Context(a.device)
    model = train_fragment_model(T, F, tseq_ptr, tseq, rev, no_bias=a.no_bias, num_training_reads=a.num_training_reads,
                                 alt_frag_model=a.alt_frag_model, seed=a.seed, assign=a.assign, mixture=a.mixture, ctx=ctx)
    save_model(a.output, model)
    fm = model["bias"] or model["fragmodel"]
    print("fragment model: %d training fragments, strand specificity %.4f, median fragment length %d%s -> %s" % (
        len(model["diagnostics"]["indices"]), fm["strand_specificity"], fm["fraglen_median"],
        "" if model["bias"] is None else ", bias model accuracy %.4f" % model["bias"]["accuracy"], a.output))
    return 0


if __name__ == "__main__":
    sys.exit(main())
