"""Restatement of the reference's splicing features in NumPy and plain Python, written straight from the Julia: splicing_features
(src/splicing.jl:98-230) over get_introns, get_cassette_exons, get_alt_donor_acceptor_sites and get_alt_fp_tp_ends
(src/transcripts.jl:545-950), the feature table as write_splicing_features_to_gene_db fills it (src/splicing.jl:233-439).

Dictionaries keyed by the intervals stand for the reference's interval collections, and the overlap join is the brute-force comparison
of every exon with every exon of its sequence and strand -- deliberately not the sort-based derivation of polee_splice_run.  The
result is put into the project's order (include/polee_hip.h) at the end; the reference's own order is that of its interval trees and
Dicts and is not reproduced.

This is the oracle of tests/test_splicing_host.py and tests/test_gpu_splicing.py.  No Julia runs in this project's tests: the expected
values are SELF-GENERATED from this restatement, not recorded from the reference."""
import numpy as np

TYPE_NAMES = ["cassette_exon", "mutex_exon", "alt_acceptor_site", "alt_donor_site", "retained_intron", "alt_5p_end", "alt_3p_end"]
STRAND_POS = 1
MERGE_DISTANCE = 250


def _transcripts(T):
    ptr = np.asarray(T["exon_ptr"], np.int64)
    first, last = np.asarray(T["exon_first"], np.int64), np.asarray(T["exon_last"], np.int64)
    out = []
    for t in range(int(T["n"])):
        exons = [(int(first[e]), int(last[e])) for e in range(ptr[t], ptr[t + 1])]
        out.append((t + 1, int(T["seq"][t]), int(T["strand"][t]), exons))
    return out


def merge_adjacent(xs, d):
    xs = sorted(xs)
    ys = [[xs[0]]]
    for x in xs[1:]:
        if x - ys[-1][-1] <= d:
            ys[-1].append(x)
        else:
            ys.append([x])
    return ys


def splicing_features(T, gene_of=None):
    """-> dict(num_features, type, seq, strand, coords [F,4], end_span [F,2], included_ptr, included_idx, excluded_ptr, excluded_idx,
    feature_idxs, feature_transcript_idxs, antifeature_idxs, antifeature_transcript_idxs, stats)"""
    ts = _transcripts(T)
    stats = dict(dropped_mutex_groups=0, features_with_repeated_members=0)

    # get_introns
    introns = {}
    for tid, seq, strand, exons in ts:
        for i in range(1, len(exons)):
            introns.setdefault((seq, strand, exons[i - 1][1] + 1, exons[i][0] - 1), []).append(tid)

    # get_cassette_exons
    flanking = {}
    for tid, seq, strand, exons in ts:
        for i in range(2, len(exons)):
            e1, e2, e3 = exons[i - 2], exons[i - 1], exons[i]
            flanking.setdefault((seq, strand, e1[1] + 1, e3[0] - 1, e2[0], e2[1]), []).append(tid)
    feats = []  # (block, order key, type, seq, strand, coords, span, included, excluded)
    for key, tids in flanking.items():
        intron = introns.get(key[:4])
        if intron is not None:
            seq, strand, f, l, ef, el = key
            feats.append((0, (seq, strand, ef, el, f, l), 0, seq, strand, (ef, el, f, l), (-1, -1), tids, intron))
    by_flanks = {}
    for key, tids in flanking.items():
        by_flanks.setdefault(key[:4], []).append((key[4], key[5], tids))
    for key, exons in by_flanks.items():
        if len(exons) <= 1:
            continue
        exons.sort(key=lambda e: (e[0], e[1]))
        flat = []
        for first, last, tids in exons:
            if not flat or first > flat[-1][1]:
                flat.append((first, last, list(tids)))
            else:
                flat[-1] = (min(flat[-1][0], first), max(flat[-1][1], last), flat[-1][2] + list(tids))
        if len(flat) <= 1:
            continue
        if len(flat) == 2:
            (fa, la, ta), (fb, lb, tb) = flat
            seq, strand = key[0], key[1]
            feats.append((1, (seq, strand, fa, la, fb, lb, key[2], key[3]), 1, seq, strand, (fa, la, fb, lb), (-1, -1), ta, tb))
        else:
            stats["dropped_mutex_groups"] += 1

    # get_alt_donor_acceptor_sites: every exon against every exon of its sequence and strand
    groups = {}
    for tid, seq, strand, exons in ts:
        for i, (f, l) in enumerate(exons):
            m2 = None if i == 0 else exons[i - 1][1] + 1
            m3 = None if i == len(exons) - 1 else exons[i + 1][0] - 1
            groups.setdefault((seq, strand), []).append((f, l, tid, m2, m3))
    alt_sites, retained = {}, {}
    pushes = {}
    for (seq, strand), ex in groups.items():
        # ("skip exons without flanks for now", transcripts.jl:700-704: the test on both exons of a pair, made before the pairs are formed)
        ex = [e for e in ex if e[3] is not None and e[4] is not None]
        if not ex:
            continue
        firsts, lasts = np.array([e[0] for e in ex], np.int64), np.array([e[1] for e in ex], np.int64)
        for a in ex:
            for j in np.nonzero((firsts <= a[1]) & (lasts >= a[0]))[0]:
                b = ex[j]
                if a[3] is None or a[4] is None or b[3] is None or b[4] is None:
                    continue
                af, al, atid, am2, am3 = a
                bf, bl, btid, bm2, bm3 = b
                alt = ri = None
                if am3 == bm3 and al != bl:
                    if al < bl:
                        alt = (al + 1, am3, bl + 1, am3, atid, btid)
                    else:
                        alt = (bl + 1, am3, al + 1, am3, btid, atid)
                elif am2 == bm2 and af != bf:
                    if af > bf:
                        alt = (am2, bf - 1, am2, af - 1, btid, atid)
                    else:
                        alt = (am2, af - 1, am2, bf - 1, atid, btid)
                elif am3 < bl:
                    ri = (al + 1, am3, btid, atid)
                elif bm3 < al:
                    ri = (bl + 1, bm3, atid, btid)
                elif am2 > bf:
                    ri = (am2, af - 1, btid, atid)
                elif bm2 > al:  # (as written, transcripts.jl:780)
                    ri = (bm2, bf - 1, atid, btid)
                if alt is not None:
                    key, inc, exc = (seq, strand) + alt[:4], alt[4], alt[5]
                    table = alt_sites
                elif ri is not None:
                    key, inc, exc = (seq, strand) + ri[:2], ri[2], ri[3]
                    table = retained
                else:
                    continue
                assert inc != exc
                entry = table.setdefault(key, (set(), set()))
                if inc in entry[0] or exc in entry[1]:
                    pushes[key] = True
                entry[0].add(inc)
                entry[1].add(exc)
    stats["features_with_repeated_members"] = len(pushes)
    for key, (inc, exc) in alt_sites.items():
        seq, strand, sf, sl, lf, ll = key
        if sf == lf:
            typ = 2 if strand == STRAND_POS else 3
        else:
            typ = 3 if strand == STRAND_POS else 2
        feats.append((2, key, typ, seq, strand, (sf, sl, lf, ll), (-1, -1), inc, exc))
    for key, (inc, exc) in retained.items():
        seq, strand, f, l = key
        feats.append((3, key, 4, seq, strand, (f, l, -1, -1), (-1, -1), inc, exc))

    # get_alt_fp_tp_ends
    if gene_of is not None:
        by_gene = {}
        for t in ts:
            by_gene.setdefault(int(gene_of[t[0] - 1]), []).append(t)
        for gene, gts in by_gene.items():
            if len(gts) <= 1:
                continue
            firsts_set = {t[3][0][0] for t in gts}
            lasts_set = {t[3][-1][1] for t in gts}
            min_first, max_last = min(firsts_set), min(lasts_set)  # (:883-884, as written)
            seq, strand = gts[0][1], gts[0][2]
            for kind, clusters in ((0, merge_adjacent(list(firsts_set), MERGE_DISTANCE)), (1, merge_adjacent(list(lasts_set), MERGE_DISTANCE))):
                if len(clusters) <= 1:
                    continue
                for cluster in clusters:
                    inc, exc = [], []
                    for t in gts:
                        x = t[3][0][0] if kind == 0 else t[3][-1][1]
                        (inc if x in cluster else exc).append(t[0])
                    fp = (strand == STRAND_POS) == (kind == 0)
                    feats.append((4 if fp else 5, (gene, kind, cluster[0]), 5 if fp else 6, seq, strand, (cluster[0], cluster[-1], -1, -1),
                                  (min_first, max_last), inc, exc))
                    if len(clusters) == 2:
                        break

    feats.sort(key=lambda f: (f[0], f[1]))
    F = len(feats)
    out = dict(num_features=F, type=np.array([f[2] for f in feats], np.int32), seq=np.array([f[3] for f in feats], np.int32),
               strand=np.array([f[4] for f in feats], np.int8), coords=np.array([f[5] for f in feats], np.int64).reshape(F, 4),
               end_span=np.array([f[6] for f in feats], np.int64).reshape(F, 2), stats=stats)
    for name, col in (("included", 7), ("excluded", 8)):
        members = [sorted(set(f[col])) for f in feats]
        out[name + "_ptr"] = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int64)
        out[name + "_idx"] = np.array([t for m in members for t in m], np.int32)
    out.update(index_vectors(out))
    return out


def index_vectors(r):
    """the four 1-based vectors splicing_features returns (src/splicing.jl:125-229) from the two CSR lists"""
    out = {}
    for name, a, b in (("included", "feature_idxs", "feature_transcript_idxs"), ("excluded", "antifeature_idxs", "antifeature_transcript_idxs")):
        ptr = np.asarray(r[name + "_ptr"], np.int64)
        out[a] = np.repeat(np.arange(1, len(ptr), dtype=np.int32), np.diff(ptr))
        out[b] = np.asarray(r[name + "_idx"], np.int32)
    return out


ARRAYS = ["type", "seq", "strand", "coords", "end_span", "included_ptr", "included_idx", "excluded_ptr", "excluded_idx", "feature_idxs",
          "feature_transcript_idxs", "antifeature_idxs", "antifeature_transcript_idxs"]


def assert_same(got, want, what=""):
    assert int(got["num_features"]) == int(want["num_features"]), (what, got["num_features"], want["num_features"])
    for k in ARRAYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and np.array_equal(g, w), (what, k, g[:12], w[:12])


# ---- inputs
def annotation(transcripts, genes=None):
    """[(seq, strand, [(first, last), ...]), ...] -> the arrays of polee_xb_transcripts (+ gene_of)"""
    ptr = np.concatenate([[0], np.cumsum([len(t[2]) for t in transcripts])]).astype(np.int64)
    ex = [e for t in transcripts for e in t[2]]
    T = dict(n=len(transcripts), seq=np.array([t[0] for t in transcripts], np.int32), strand=np.array([t[1] for t in transcripts], np.int8),
             exon_ptr=ptr, exon_first=np.array([e[0] for e in ex], np.int64), exon_last=np.array([e[1] for e in ex], np.int64))
    if genes is not None:
        T["gene_of"] = np.asarray(genes, np.int32)
    return T


def concatenate(parts):
    """several annotations as one: genes renumbered part by part (sequences and coordinates stay)"""
    ts, genes, g0 = [], [], 0
    for T in parts:
        ptr = T["exon_ptr"]
        for t in range(T["n"]):
            ts.append((int(T["seq"][t]), int(T["strand"][t]), [(int(T["exon_first"][e]), int(T["exon_last"][e])) for e in range(ptr[t], ptr[t + 1])]))
        g = np.asarray(T["gene_of"] if "gene_of" in T else np.arange(1, T["n"] + 1))
        genes += list(g + g0)
        g0 += int(g.max())
    return annotation(ts, genes)


def hand_made_loci():
    """{name: annotation}: one locus per rule and per quirk, every one on both strands (the second copy on another sequence so that the
    two do not meet).  Exons of a locus are written on the plus strand; the minus-strand copy has the same coordinates."""
    L = {}
    A, B, C, D = (100, 200), (300, 400), (500, 600), (700, 800)

    def both(name, isoforms, genes=None):
        ts = [(0, 1, iso) for iso in isoforms] + [(1, -1, iso) for iso in isoforms]
        g = None if genes is None else list(genes) + [x + max(genes) for x in genes]
        L[name] = annotation(ts, g if g is not None else [1] * len(isoforms) + [2] * len(isoforms))
    both("cassette", [[A, B, C], [A, C]])
    both("mutex_two_unions", [[A, B, D], [A, C, D]])
    both("mutex_three_unions", [[A, (300, 340), D], [A, (400, 440), D], [A, (500, 540), D]])
    both("mutex_merging", [[A, (300, 400), D], [A, (350, 450), D], [A, (500, 600), D]])
    # alternative sites: case 1 (the same following intron end), case 2 (the same preceding intron start), both size orders by the
    # order of the transcripts
    both("alt_case1_short_first", [[A, (300, 380), D], [A, (300, 420), D]])
    both("alt_case1_long_first", [[A, (300, 420), D], [A, (300, 380), D]])
    both("alt_case2_short_first", [[A, (330, 400), D], [A, (300, 400), D]])
    both("alt_case2_long_first", [[A, (300, 400), D], [A, (330, 400), D]])
    # retained introns.  (300, 350) of the first transcript against (300, 520) of the second: its following intron (351, 449) lies inside
    # the other exon -- the first branch in one order, the second in the other; (450, 500) against (300, 520): its preceding intron does,
    # the third branch
    both("retained_following_and_preceding", [[A, (300, 350), (450, 500), D], [(50, 90), (300, 520), (900, 950)]])
    # the third branch alone: (300, 350) is a first exon here, so only (450, 500) meets (320, 470), which covers its preceding intron
    both("retained_preceding_only", [[(300, 350), (450, 500), (700, 800), (900, 950)], [(50, 90), (320, 470), (990, 999)]])
    # the last branch (transcripts.jl:780) asks b.metadata[2] > a.last where the drawing suggests a.first.  With a = (250, 365) of the
    # first transcript and b = (360, 420) of the second (preceding intron from 291) no earlier branch fires, 291 > 365 is false as
    # written and 291 > 250 would be true.  (As written the branch can never fire for overlapping exons -- b.metadata[2] <= b.first <=
    # a.last -- and the retained intron (291, 359) still comes out of the pair's other order, through the third branch.)
    both("line_780_as_written", [[(100, 200), (250, 365), (600, 700)], [(100, 290), (360, 420), (650, 700)]])
    both("no_branch", [[(100, 200), (300, 400), (700, 800)], [(150, 200), (300, 400), (700, 850)]])
    both("single_exon", [[A], [(150, 900)]])
    both("two_exons", [[A, B], [A, (320, 400)]])
    both("identical_transcripts", [[A, B, C], [A, B, C], [A, C], [A, C], [A, (300, 380), C]])
    L["other_seq_or_strand"] = annotation([(0, 1, [A, B, C]), (1, 1, [A, C]), (0, -1, [A, C]), (2, 1, [A, (300, 380), D]), (2, -1, [A, (300, 420), D])],
                                          [1, 1, 1, 2, 2])
    both("ends_one_cluster", [[(100, 200), D], [(120, 200), (700, 820)]])
    both("ends_two_clusters", [[(100, 200), D], [(400, 450), D], [(120, 200), D]])
    both("ends_three_clusters", [[(100, 200), (5000, 5100)], [(1000, 1100), (5000, 5500)], [(2000, 2100), (5000, 6000)], [(2100, 2200), (5000, 6100)]])
    both("ends_250_apart", [[(100, 200), D], [(350, 400), D]])
    both("ends_251_apart", [[(100, 200), D], [(351, 400), D]])
    both("ends_min_differs_from_max", [[(100, 200), (700, 800)], [(100, 200), (700, 1500)], [(900, 950), (1400, 1600)]])
    both("no_features", [[A, B, C], [(1000, 1100), (1200, 1300), (1400, 1500)]], genes=[1, 2])
    return L
