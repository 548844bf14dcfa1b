"""Splicing features from the transcripts' exon structure on the GPU (polee_splice_*): the reference's
`splicing_features` (src/splicing.jl:98-230) over get_introns, get_cassette_exons, get_alt_donor_acceptor_sites and get_alt_fp_tp_ends
(src/transcripts.jl:545-950) -- cassette and mutually exclusive exons, alternative donor / acceptor sites, retained introns and, with
the transcripts' genes, alternative 5' and 3' ends -- and what src/regression.jl:527-549 does with them before the model.

    python -m polee_amd.splicing transcripts.npz -o splicing-features.npz [--table features.csv] [--host] [--device D]
        [--alt-ends --transcript-ids ids.txt (--gene-pattern RX | --gene-annotations genes.yml)]
        [--experiment experiment.yml [--transformation tree.h5] [--approx-output splicing-approx.csv] [--seed N]]

transcripts.npz holds the arrays of polee_xb_transcripts under the names alignments.npz uses: t_seq, t_strand, exon_ptr, exon_first,
exon_last (1-based inclusive coordinates up to 2^31 - 2, exons ascending and disjoint).  The order of the features is this project's
own (include/polee_hip.h).  POLEE_BUILD_TIMING=1: the phases on stderr."""
import argparse
import ctypes as C
import sys

import numpy as np

from . import _lib as L
from ._lib import check
from .xbuild import _T_TYPES, _Transcripts

TYPE_NAMES = ["cassette_exon", "mutex_exon", "alt_acceptor_site", "alt_donor_site", "retained_intron", "alt_5p_end", "alt_3p_end"]


class _Splice(L.Handle):
    _destroy = "polee_splice_destroy"

    def __init__(self, h):
        self._h = h


def splicing_features(transcripts, gene_of=None, host=False, ctx=None):
    """transcripts: dict(n, seq, strand, exon_ptr, exon_first, exon_last); gene_of: i32 [n], 1-based, or None = no alternative ends.
    -> dict(num_features, type i32 [F] (index into TYPE_NAMES), seq, strand, coords i64 [F, 4] (included_first, included_last,
    excluded_first, excluded_last; -1 where the reference's table holds -1), end_span i64 [F, 2] (an alternative end's min_first and
    max_last as upstream computes them), included_ptr / included_idx, excluded_ptr / excluded_idx (CSR, transcripts 1-based, ascending
    and unique), the four 1-based vectors of the reference -- feature_idxs, feature_transcript_idxs, antifeature_idxs,
    antifeature_transcript_idxs -- and num_exons, num_internal_exons, num_overlapping_pairs).  host: on the host threads, no GPU."""
    lib = L.lib()
    keep = [np.ascontiguousarray(transcripts[k], dt) for k, dt in _T_TYPES.items()]
    n = int(transcripts["n"])
    if len(keep[0]) != n or len(keep[1]) != n or len(keep[2]) != n + 1 or len(keep[3]) != len(keep[4]) or \
            (n > 0 and len(keep[3]) < int(keep[2][-1])):
        raise ValueError("the transcripts' arrays do not have the sizes n, n, n + 1 and exon_ptr[n]")
    T = _Transcripts(n, *[a.ctypes.data_as(C.c_void_p) for a in keep])
    g = None
    if gene_of is not None:
        g = np.ascontiguousarray(gene_of, np.int32)
        if g.shape != (n,):
            raise ValueError("gene_of must hold one gene number per transcript")
    gp = None if g is None else g.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    if host:
        check(lib.polee_splice_run_host(C.byref(T), gp, C.byref(h)))
    else:
        from .core import default_context
        ctx = ctx or default_context()
        check(lib.polee_splice_run(ctx._h, C.byref(T), gp, C.byref(h)), ctx._h)
    owner = _Splice(h)
    try:
        sizes = [C.c_int64() for _ in range(6)]
        check(lib.polee_splice_sizes(h, *[C.byref(s) for s in sizes]))
        F, ni, ne = (s.value for s in sizes[:3])
        out = dict(num_features=F, type=np.empty(F, np.int32), seq=np.empty(F, np.int32), strand=np.empty(F, np.int8),
                   coords=np.empty((F, 4), np.int64), end_span=np.empty((F, 2), np.int64), included_ptr=np.empty(F + 1, np.int64),
                   included_idx=np.empty(ni, np.int32), excluded_ptr=np.empty(F + 1, np.int64), excluded_idx=np.empty(ne, np.int32))
        check(lib.polee_splice_get(h, *[out[k].ctypes.data_as(C.c_void_p) for k in
                                        ("type", "seq", "strand", "coords", "end_span", "included_ptr", "included_idx", "excluded_ptr",
                                         "excluded_idx")]))
        out.update(num_exons=sizes[3].value, num_internal_exons=sizes[4].value, num_overlapping_pairs=sizes[5].value)
    finally:
        owner.close()
    out["feature_idxs"] = np.repeat(np.arange(1, F + 1, dtype=np.int32), np.diff(out["included_ptr"]))
    out["feature_transcript_idxs"] = out["included_idx"]
    out["antifeature_idxs"] = np.repeat(np.arange(1, F + 1, dtype=np.int32), np.diff(out["excluded_ptr"]))
    out["antifeature_transcript_idxs"] = out["excluded_idx"]
    return out


def feature_initial_values(x0, r):
    """x_init = log sum_included x0 - log sum_excluded x0, f32 [S, F] (src/regression.jl:527-543: Float32 sums in the pairs' order);
    a non-finite entry is an error that names the feature (the reference asserts)."""
    x0 = np.asarray(x0, np.float32)
    S, F = x0.shape[0], int(r["num_features"])
    num, den = np.zeros((S, F), np.float32), np.zeros((S, F), np.float32)
    for k in range(S):
        np.add.at(num[k], r["feature_idxs"] - 1, x0[k, r["feature_transcript_idxs"] - 1])
        np.add.at(den[k], r["antifeature_idxs"] - 1, x0[k, r["antifeature_transcript_idxs"] - 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        x_init = np.log(num) - np.log(den)
    bad = np.argwhere(~np.isfinite(x_init))
    if bad.size:
        k, f = (int(v) for v in bad[0])
        raise ValueError("the initial value of feature %d (%s, sequence %d, %d-%d) is not finite in sample %d: its included or its "
                         "excluded transcripts have no expression there" % (f + 1, TYPE_NAMES[int(r["type"][f])], int(r["seq"][f]),
                                                                            int(r["coords"][f, 0]), int(r["coords"][f, 1]), k + 1))
    return x_init


def read_transcripts(filename):
    with np.load(filename) as z:
        names = dict(seq="t_seq" if "t_seq" in z.files else "seq", strand="t_strand" if "t_strand" in z.files else "strand",
                     exon_ptr="exon_ptr", exon_first="exon_first", exon_last="exon_last")
        missing = [v for v in names.values() if v not in z.files]
        if missing:
            raise SystemExit("%s lacks %s" % (filename, ", ".join(missing)))
        T = {k: z[v] for k, v in names.items()}
    T["n"] = len(T["seq"])
    return T


def write_table(filename, r):
    """the reference's splicing_features table (src/splicing.jl:240-250), one row per feature"""
    with open(filename, "w") as f:
        f.write("feature_num,type,seqname,strand,included_first,included_last,excluded_first,excluded_last\n")
        for i in range(int(r["num_features"])):
            f.write("%d,%s,%d,%d,%d,%d,%d,%d\n" % ((i + 1, TYPE_NAMES[int(r["type"][i])], int(r["seq"][i]), int(r["strand"][i]))
                                                   + tuple(int(v) for v in r["coords"][i])))


def parser():
    ap = argparse.ArgumentParser(prog="python -m polee_amd.splicing", description=__doc__.split("\n\n")[0])
    ap.add_argument("transcripts", metavar="transcripts.npz")
    ap.add_argument("--output", "-o", default="splicing-features.npz")
    ap.add_argument("--table", metavar="features.csv", help="Write the feature table, one row per feature.")
    ap.add_argument("--alt-ends", action="store_true", help="Alternative 5' and 3' ends too (needs the transcripts' genes).")
    ap.add_argument("--gene-pattern", metavar="RX")
    ap.add_argument("--gene-annotations", metavar="genes.yml")
    ap.add_argument("--transcript-ids", metavar="ids.txt", help="Transcript ids, one per line.")
    ap.add_argument("--host", action="store_true", help="Derive the features on the host threads, without a GPU.")
    ap.add_argument("--device", type=int, default=0, metavar="D", help="GPU to run on")
    ap.add_argument("--experiment", metavar="experiment.yml",
                    help="Also: initial values and the normal approximation of the splicing log-ratios of the experiment's samples.")
    ap.add_argument("--transformation", metavar="tree.h5", help="With --experiment: the tree of the prepared samples, as for `model regression`.")
    ap.add_argument("--approx-output", default="splicing-approx.csv", metavar="splicing-approx.csv", help="With --experiment: where loc and scale go.")
    ap.add_argument("--seed", type=int, default=123456789, help="With --experiment: the seed of the draws behind loc and scale.")
    return ap


def main(argv=None):
    a = parser().parse_args(sys.argv[1:] if argv is None else argv)
    T = read_transcripts(a.transcripts)
    gene_of = None
    if a.alt_ends:
        if (a.gene_pattern is None) == (a.gene_annotations is None):
            raise SystemExit("--alt-ends needs exactly one of --gene-pattern and --gene-annotations")
        if not a.transcript_ids:
            raise SystemExit("--alt-ends needs --transcript-ids: genes are found from the transcripts' ids")
        from .pca import read_experiment
        from .regression import gene_map
        from .sample import _read_lines
        ids = _read_lines(a.transcript_ids)
        if len(ids) != T["n"]:
            raise SystemExit("%s names %d transcripts, %s holds %d" % (a.transcript_ids, len(ids), a.transcripts, T["n"]))
        annotations = None if a.gene_annotations is None else read_experiment(a.gene_annotations)
        try:
            _, gene_idxs, _, _, _ = gene_map(ids, a.gene_pattern, annotations)
        except ValueError as e:
            raise SystemExit(str(e))
        gene_of = gene_idxs.astype(np.int32)
    ctx = None
    if not a.host or a.experiment:
        from .core import Context
        ctx = Context(a.device)
    try:
        r = splicing_features(T, gene_of, host=a.host, ctx=ctx)
    except L.PoleeError as e:
        raise SystemExit(str(e.args[-1]))
    counts = np.bincount(r["type"], minlength=len(TYPE_NAMES))
    print("Read %d cassette exons\n     %d mutually exclusive exons\n     %d alternate acceptor/donor sites\n     %d retained introns"
          % (counts[0], counts[1], counts[2] + counts[3], counts[4]))
    if a.alt_ends:
        print("     %d alternate 5' ends\n     %d alternate 3' ends" % (counts[5], counts[6]))
    extra = {}
    if a.experiment:
        from . import estimate
        from .pca import read_experiment
        spec = read_experiment(a.experiment)
        if not spec.get("samples"):
            raise SystemExit("%s names no samples" % a.experiment)
        ls = estimate.load_samples_from_specification(spec, T["n"], ptt_filename=a.transformation, ctx=ctx)
        try:
            extra["x_init"] = feature_initial_values(ls.x0_values, r)
        except ValueError as e:
            raise SystemExit(str(e))
        F = int(r["num_features"])
        loc, scale = ls.variables["approx"].approximate_splicing_likelihood(
            F, np.stack([r["feature_idxs"] - 1, r["feature_transcript_idxs"] - 1], axis=1),
            np.stack([r["antifeature_idxs"] - 1, r["antifeature_transcript_idxs"] - 1], axis=1), seed=a.seed)
        extra.update(qx_feature_loc=loc, qx_feature_scale=scale)
        with open(a.approx_output, "w") as f:  # (src/splicing.jl:76-81)
            f.write("i,j,loc,scale\n")
            for i in range(loc.shape[0]):
                for j in range(F):
                    f.write("%d,%d,%r,%r\n" % (i + 1, j + 1, float(loc[i, j]), float(scale[i, j])))
    np.savez(a.output, type_names=np.array(TYPE_NAMES), **{k: v for k, v in r.items()}, **extra)
    if a.table:
        write_table(a.table, r)
    return 0


if __name__ == "__main__":
    sys.exit(main())
