// `polee model random-forest` (models/random-forest.jl): the forest of DESIGN.md section 3.14 (definitions: forest_common.hpp) grown
// on the device, level by level for all trees at once, and its prediction.
//
// Training rows live feature-major, xT [n][N], so the gather of a node's rows from one feature stays inside one run of 4 N bytes.
// Every tree keeps its bootstrap rows in an array [N_b]; every node owns a contiguous segment of it.  Per level, on the context's
// stream:
//   1. forest_search_wave_kernel    nodes of <= 64 rows: one wave per (node, chunk of candidates), no barrier.  The wave sorts
//                                   (sortable value bits, label) by lane exchanges, takes per-class prefix counts by ballot and
//                                   popcount below the lane, scores the boundary in front of every lane and reduces by shuffles.
//      forest_search_block_kernel   larger nodes: one workgroup per (node, chunk); bitonic sort in LDS (1024 or 8192 slots), per-class
//                                   running counts from a packed block scan, every thread scores a contiguous run of boundaries.
//      Output: one best (score, position, boundary) per (node, chunk); chunk 0 also writes the node's class counts.
//   2. forest_pick_kernel           one workgroup per tree: reduces the chunks of each of its open nodes (the lexicographic maximum does
//                                   not depend on the order), decides leaf or split, numbers the children by a prefix sum and writes
//                                   the node records.
//      forest_level_scan_kernel     prefix sum over the trees: where each tree's children stand in the next level's node list.
//   3. forest_partition_kernel      one wave per split node: stable partition of its row segment into left | right (into the other of
//                                   two row arrays) and the two entries of the next level's list.
// The host reads one small record per level (open nodes and how many of them each search kernel takes) and stops at zero.
// There are no float atomics; the only atomics append node indices to the search kernels' work lists, whose order changes nothing.
// Compiled with -ffp-contract=off: the score is a chain of f64 additions that the host builder repeats bit for bit.
#include "draw_model.hpp"  // check_approx, check_points, DrawFeed
#include "forest_common.hpp"

namespace polee {
namespace forest {

constexpr int FO_BLOCK = 256;
constexpr int FO_WAVES = FO_BLOCK / 64;
constexpr int FO_MIN_CHUNK = 16;          // fewest candidates of one work item
constexpr int64_t FO_TARGET_ITEMS = 1 << 15;  // work items a level is cut into when it has few open nodes
constexpr int FO_MID = 1024;              // sort slots of the smaller workgroup kernel
constexpr int FO_MAX_N_ROWS = 1 << 27;    // (row, label) pack into 32 bits

struct OpenNode {
    int32_t tree, node, beg, end, depth;  // rows [beg, end) of the tree's row array
};
struct Best {
    double score;
    float lo, hi;  // the two values the boundary lies between
    int32_t pos;   // candidate position, -1: no valid boundary
    int32_t feat, nl, pad;
};
// what a level's kernels share (device pointers)
struct Level {
    const float *xT;
    const uint8_t *labels;
    const double *T;
    const int32_t *rows;  // [ntrees][Nb], this level's
    int32_t *rows_next;
    const OpenNode *open;
    OpenNode *open_next;
    const int32_t *tstart;  // [ntrees + 1]: first open node of every tree
    int32_t *tstart_next;
    const int32_t *lists;  // [3][cap]: open nodes of <= 64, <= FO_MID, more rows
    int32_t *lists_next;
    int32_t *rec;  // next level: open nodes, then the three list lengths
    Best *best;    // [open][nchunks]
    int32_t *counts;  // [open][FO_MAX_K]
    int32_t *dec_child, *dec_slot, *dec_feat, *dec_nl;  // per open node: first child's number (-1: leaf), its slot in the next list
    double *dec_thr;
    int32_t *tree_nodes, *nsplit;  // [ntrees]
    int32_t *feature, *left, *right, *label;  // [ntrees][maxn]
    double *threshold;
    int64_t N, cap;
    uint64_t seed;
    int32_t n, k, Nb, ntrees, maxn, nsub, nchunks, csize, max_depth, min_leaf, min_split;
};

__device__ inline float bits_float(uint32_t u) { return __uint_as_float(u); }

__device__ inline bool trivial_leaf(const int32_t *tot, int k, int32_t cnt, int32_t depth, const Level &p)
{
    int32_t mx = 0;
    for (int c = 0; c < k; ++c) mx = max(mx, tot[c]);
    return mx == cnt || cnt < p.min_split || depth == p.max_depth;
}

// The log of a draw: taken in f64 and rounded once, so within half an ulp of f32 (and a bit) of the true log.  Device logf (the
// hardware's log2 times ln 2) was measured more than one ulp from the f64 log, and two f32 steps from its rounding, on the draws of
// tests/test_gpu_forest.py, where |log x| ~ 10.  The rows are what every builder and the tests see (polee_forest_log_draws), so the
// choice changes no comparison between builders, only how close the rows are to the host's log.
__device__ inline float log_f32(float v) { return (float)log((double)v); }

// ---- layout ---------------------------------------------------------------------------------------------------------------------
// in [R][n] -> xT[j][r0 + r], through a 32 x 32 LDS tile; take_log: the log of the (clipped, positive) draw
__global__ __launch_bounds__(256) void forest_layout_kernel(const float *__restrict__ in, int32_t R, int32_t n, int take_log,
                                                           float *__restrict__ xT, int64_t N, int64_t r0)
{
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t j0 = (int64_t)blockIdx.x * 32, rb = (int64_t)blockIdx.y * 32;
    for (int i = ty; i < 32; i += 8) {
        const int64_t r = rb + i, j = j0 + tx;
        if (r < R && j < n) {
            const float v = in[r * n + j];
            tile[i][tx] = take_log ? log_f32(v) : v;
        }
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int64_t j = j0 + i, r = rb + tx;
        if (r < R && j < n) xT[j * N + r0 + r] = tile[tx][i];
    }
}

__global__ void forest_log_kernel(int64_t count, const float *__restrict__ in, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = log_f32(in[i]);
}

__global__ void forest_init_kernel(Level p, int32_t *rows, OpenNode *open, int32_t *tstart, int32_t *lists, int32_t *rec)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (int64_t)p.ntrees * p.Nb) {
        const uint32_t t = (uint32_t)(i / p.Nb), e = (uint32_t)(i % p.Nb);
        rows[i] = (int32_t)boot_row(p.seed, t, e, (uint32_t)p.N);
    }
    if (i < p.ntrees) {
        open[i] = OpenNode{(int32_t)i, 0, 0, p.Nb, 0};
        tstart[i] = (int32_t)i;
        p.tree_nodes[i] = 1;
        const int cls = p.Nb <= 64 ? 0 : p.Nb <= FO_MID ? 1 : 2;
        lists[(int64_t)cls * p.cap + i] = (int32_t)i;
    }
    if (i == 0) {
        tstart[p.ntrees] = p.ntrees;
        const int cls = p.Nb <= 64 ? 0 : p.Nb <= FO_MID ? 1 : 2;
        rec[0] = p.ntrees;
        for (int c = 0; c < 3; ++c) rec[1 + c] = c == cls ? p.ntrees : 0;
    }
}

// ---- split search, nodes of <= 64 rows: one wave per (node, chunk) -----------------------------------------------------------------
template <int KP>
__global__ __launch_bounds__(FO_BLOCK) void forest_search_wave_kernel(Level p, int32_t nlist)
{
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * FO_WAVES + (threadIdx.x >> 6);
    if (item >= (int64_t)nlist * p.nchunks) return;  // (wave-uniform; the kernel has no barrier)
    const int32_t oi = p.lists[item / p.nchunks], chunk = (int32_t)(item % p.nchunks);
    const OpenNode nd = p.open[oi];
    const int32_t cnt = nd.end - nd.beg;
    const bool live = lane < cnt;
    const int32_t row = live ? p.rows[(int64_t)nd.tree * p.Nb + nd.beg + lane] : 0;
    const uint32_t lab = live ? (uint32_t)p.labels[row] : 0xFFu;
    int32_t tot[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) tot[c] = __popcll(__ballot(lab == (uint32_t)c));
    if (chunk == 0 && lane < p.k) {
        int32_t mine = 0;
#pragma unroll
        for (int c = 0; c < KP; ++c) mine = lane == c ? tot[c] : mine;
        p.counts[(int64_t)oi * FO_MAX_K + lane] = mine;
    }
    if (trivial_leaf(tot, min(p.k, KP), cnt, nd.depth, p)) return;  // (the pick kernel sees the same counts and reads no best)
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
    bool bfound = false;
    double bscore = 0.0;
    float blo = 0.0f, bhi = 0.0f;
    int32_t bpos = -1, bfeat = -1, bnl = 0;
    const int32_t pos1 = min(p.nsub, (chunk + 1) * p.csize);
    for (int32_t pos = chunk * p.csize; pos < pos1; ++pos) {
        const uint32_t f = candidate_feature(p.seed, (uint32_t)nd.tree, (uint32_t)nd.node, (uint32_t)p.n, (uint32_t)pos);
        uint64_t key = ~0ull;
        if (live) key = ((uint64_t)sortable_bits(__float_as_uint(p.xT[(int64_t)f * p.N + row])) << 32) | lab;
        // bitonic sort over the 64 lanes, ascending; the padding lanes hold the largest key
#pragma unroll
        for (int k2 = 2; k2 <= 64; k2 <<= 1)
#pragma unroll
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                const uint64_t other = __shfl_xor(key, j, 64);
                const bool up = (lane & k2) == 0, lower = (lane & j) == 0;
                key = (lower == up) ? (key < other ? key : other) : (key < other ? other : key);
            }
        const uint32_t slab = (uint32_t)key & 0xFFu;
        const float v = bits_float(unsortable_bits((uint32_t)(key >> 32)));
        const float vprev = __shfl_up(v, 1, 64);
        // the boundary in front of lane i: left = lanes 0 .. i-1
        bool valid = lane >= 1 && live && vprev < v && lane >= p.min_leaf && cnt - lane >= p.min_leaf;
        int32_t cl[KP];
#pragma unroll
        for (int c = 0; c < KP; ++c) cl[c] = __popcll(__ballot(live && slab == (uint32_t)c) & below);
        double score = 0.0;
        if (valid) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < KP; ++c)
                if (c < p.k) {
                    s += p.T[cl[c]];
                    s += p.T[tot[c] - cl[c]];
                }
            s -= p.T[lane];
            s -= p.T[cnt - lane];
            score = s;
        }
        int32_t idx = lane;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double os = __shfl_xor(score, off, 64);
            const int32_t oidx = __shfl_xor(idx, off, 64);
            const bool ov = __shfl_xor((int)valid, off, 64) != 0;
            if (ov && (!valid || os > score || (os == score && oidx < idx))) {
                valid = true;
                score = os;
                idx = oidx;
            }
        }
        if (valid && (!bfound || score > bscore)) {  // (positions ascend: a tie keeps the earlier one)
            bfound = true;
            bscore = score;
            blo = __shfl(vprev, idx, 64);
            bhi = __shfl(v, idx, 64);
            bpos = pos;
            bfeat = (int32_t)f;
            bnl = idx;
        }
    }
    if (lane == 0) p.best[(int64_t)oi * p.nchunks + chunk] = Best{bscore, blo, bhi, bpos, bfeat, bnl, 0};
}

// exclusive prefix over the workgroup's threads; *total = the sum.  s_w: FO_WAVES words of LDS, free again on return.
template <class V>
__device__ inline V block_excl_scan(V v, V *total, V *s_w)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    V inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const V t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    V base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < FO_WAVES; ++w) {
        const V x = s_w[w];
        if (w < wave) base += x;
        tot += x;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// ---- split search, larger nodes: one workgroup per (node, chunk) -------------------------------------------------------------------
template <int CAP, int KP>
__global__ __launch_bounds__(FO_BLOCK) void forest_search_block_kernel(Level p, int32_t nlist, int which)
{
    __shared__ uint64_t keys[CAP];
    __shared__ uint32_t rl[CAP];  // row << 4 | label of the node's rows, read once
    __shared__ int32_t s_tot[FO_MAX_K];
    __shared__ uint64_t s_scan[FO_WAVES];
    __shared__ double s_score[FO_WAVES];
    __shared__ int32_t s_idx[FO_WAVES];
    constexpr int NW = KP / 4;  // four 16-bit class counts per scanned word (a node has at most 8192 rows)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t item = blockIdx.x;
    const int32_t oi = p.lists[(int64_t)which * p.cap + item / p.nchunks], chunk = (int32_t)(item % p.nchunks);
    const OpenNode nd = p.open[oi];
    const int32_t cnt = nd.end - nd.beg;
    if (cnt > CAP) return;  // (cannot happen: the lists are filled by size)
    if (tid < FO_MAX_K) s_tot[tid] = 0;
    __syncthreads();
    for (int32_t j = tid; j < cnt; j += FO_BLOCK) {
        const int32_t row = p.rows[(int64_t)nd.tree * p.Nb + nd.beg + j];
        const uint32_t lab = p.labels[row];
        rl[j] = ((uint32_t)row << 4) | lab;
        atomicAdd(&s_tot[lab], 1);
    }
    __syncthreads();
    int32_t tot[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) tot[c] = s_tot[c];
    if (chunk == 0 && tid < p.k) p.counts[(int64_t)oi * FO_MAX_K + tid] = s_tot[tid];
    if (trivial_leaf(tot, min(p.k, KP), cnt, nd.depth, p)) return;  // (uniform over the workgroup)
    int32_t P = 128;
    while (P < cnt) P <<= 1;
    const int32_t per = (P + FO_BLOCK - 1) / FO_BLOCK, i0 = tid * per, i1 = min(cnt, i0 + per);
    bool bfound = false;
    double bscore = 0.0;
    float blo = 0.0f, bhi = 0.0f;
    int32_t bpos = -1, bfeat = -1, bnl = 0;
    const int32_t pos1 = min(p.nsub, (chunk + 1) * p.csize);
    for (int32_t pos = chunk * p.csize; pos < pos1; ++pos) {
        const uint32_t f = candidate_feature(p.seed, (uint32_t)nd.tree, (uint32_t)nd.node, (uint32_t)p.n, (uint32_t)pos);
        __syncthreads();  // (the last candidate's keys have been read)
        for (int32_t j = tid; j < P; j += FO_BLOCK) {
            uint64_t key = ~0ull;
            if (j < cnt) {
                const uint32_t w = rl[j];
                key = ((uint64_t)sortable_bits(__float_as_uint(p.xT[(int64_t)f * p.N + (w >> 4)])) << 32) | (w & 15u);
            }
            keys[j] = key;
        }
        __syncthreads();
        for (int32_t k2 = 2; k2 <= P; k2 <<= 1)
            for (int32_t j = k2 >> 1; j > 0; j >>= 1) {
                for (int32_t e = tid; e < (P >> 1); e += FO_BLOCK) {
                    const int32_t i = ((e & ~(j - 1)) << 1) | (e & (j - 1)), l = i | j;
                    const uint64_t a = keys[i], b = keys[l];
                    if ((a > b) == ((i & k2) == 0)) {
                        keys[i] = b;
                        keys[l] = a;
                    }
                }
                __syncthreads();
            }
        // class counts of the thread's run [i0, i1), then of everything in front of it
        uint64_t mine[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) mine[w] = 0;
        for (int32_t i = i0; i < i1; ++i) {
            const uint32_t lab = (uint32_t)keys[i] & 15u;
#pragma unroll
            for (int w = 0; w < NW; ++w) mine[w] += (lab >> 2) == (uint32_t)w ? (1ull << (16 * (lab & 3u))) : 0ull;
        }
        int32_t cl[KP];
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            uint64_t total;
            const uint64_t ex = block_excl_scan<uint64_t>(mine[w], &total, s_scan);
#pragma unroll
            for (int q = 0; q < 4; ++q) cl[4 * w + q] = (int32_t)((ex >> (16 * q)) & 0xFFFFu);
        }
        bool valid = false;
        double score = 0.0;
        int32_t idx = 0;
        for (int32_t i = i0; i < i1; ++i) {
            if (i >= 1 && i >= p.min_leaf && cnt - i >= p.min_leaf) {
                const float lo = bits_float(unsortable_bits((uint32_t)(keys[i - 1] >> 32)));
                const float hi = bits_float(unsortable_bits((uint32_t)(keys[i] >> 32)));
                if (lo < hi) {
                    double s = 0.0;
#pragma unroll
                    for (int c = 0; c < KP; ++c)
                        if (c < p.k) {
                            s += p.T[cl[c]];
                            s += p.T[tot[c] - cl[c]];
                        }
                    s -= p.T[i];
                    s -= p.T[cnt - i];
                    if (!valid || s > score) {  // (boundaries ascend: a tie keeps the smaller threshold)
                        valid = true;
                        score = s;
                        idx = i;
                    }
                }
            }
            const uint32_t lab = (uint32_t)keys[i] & 15u;
#pragma unroll
            for (int c = 0; c < KP; ++c) cl[c] += lab == (uint32_t)c ? 1 : 0;
        }
        if (!valid) idx = 0x7FFFFFFF;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double os = __shfl_xor(score, off, 64);
            const int32_t oidx = __shfl_xor(idx, off, 64);
            const bool ov = oidx != 0x7FFFFFFF;
            if (ov && (!valid || os > score || (os == score && oidx < idx))) {
                valid = true;
                score = os;
                idx = oidx;
            }
        }
        if (lane == 0) {
            s_score[wave] = score;
            s_idx[wave] = idx;
        }
        __syncthreads();
        valid = false;
#pragma unroll
        for (int w = 0; w < FO_WAVES; ++w) {
            const double os = s_score[w];
            const int32_t oidx = s_idx[w];
            if (oidx != 0x7FFFFFFF && (!valid || os > score || (os == score && oidx < idx))) {
                valid = true;
                score = os;
                idx = oidx;
            }
        }
        if (valid && (!bfound || score > bscore)) {
            bfound = true;
            bscore = score;
            blo = bits_float(unsortable_bits((uint32_t)(keys[idx - 1] >> 32)));
            bhi = bits_float(unsortable_bits((uint32_t)(keys[idx] >> 32)));
            bpos = pos;
            bfeat = (int32_t)f;
            bnl = idx;
        }
    }
    if (tid == 0) p.best[(int64_t)oi * p.nchunks + chunk] = Best{bscore, blo, bhi, bpos, bfeat, bnl, 0};
}

// ---- pick: one workgroup per tree ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FO_BLOCK) void forest_pick_kernel(Level p)
{
    __shared__ int32_t s_scan[FO_WAVES];
    const int tid = threadIdx.x, t = blockIdx.x;
    const int32_t o0 = p.tstart[t], o1 = p.tstart[t + 1];
    const int32_t base = p.tree_nodes[t];
    int32_t carry = 0;
    for (int32_t ob = o0; ob < o1; ob += FO_BLOCK) {  // (uniform trip count: the scan has barriers)
        const int32_t oi = ob + tid;
        const bool live = oi < o1;
        OpenNode nd{};
        Best b{};
        b.pos = -1;
        int32_t lab = 0;
        if (live) {
            nd = p.open[oi];
            const int32_t cnt = nd.end - nd.beg;
            int32_t tot[FO_MAX_K];
            for (int c = 0; c < p.k; ++c) tot[c] = p.counts[(int64_t)oi * FO_MAX_K + c];
            for (int c = 1; c < p.k; ++c)
                if (tot[c] > tot[lab]) lab = c;
            if (!trivial_leaf(tot, p.k, cnt, nd.depth, p))
                for (int32_t ch = 0; ch < p.nchunks; ++ch) {
                    const Best o = p.best[(int64_t)oi * p.nchunks + ch];
                    if (o.pos >= 0 && (b.pos < 0 || o.score > b.score || (o.score == b.score && o.pos < b.pos))) b = o;
                }
            // (both children of a boundary are non-empty; the node arrays and the level lists are sized by that)
            if (b.pos >= 0 && (b.nl < 1 || b.nl >= cnt)) b.pos = -1;
        }
        const int32_t split = live && b.pos >= 0 ? 1 : 0;
        int32_t total;
        const int32_t pref = carry + block_excl_scan<int32_t>(split, &total, s_scan);
        carry += total;
        if (live) {
            const int64_t at = (int64_t)t * p.maxn + nd.node;
            const int32_t child = base + 2 * pref;
            const double thr = split ? threshold_of(b.lo, b.hi) : 0.0;
            p.feature[at] = split ? b.feat : -1;
            p.threshold[at] = thr;
            p.left[at] = split ? child : -1;
            p.right[at] = split ? child + 1 : -1;
            p.label[at] = lab;
            p.dec_child[oi] = split ? child : -1;
            p.dec_slot[oi] = 2 * pref;
            p.dec_feat[oi] = b.feat;
            p.dec_nl[oi] = b.nl;
            p.dec_thr[oi] = thr;
        }
    }
    if (tid == 0) {
        p.nsplit[t] = carry;
        p.tree_nodes[t] = base + 2 * carry;
    }
}

// one workgroup: tstart_next = the exclusive prefix of 2 nsplit over the trees; the next level's record
__global__ __launch_bounds__(FO_BLOCK) void forest_level_scan_kernel(Level p)
{
    __shared__ int32_t s_scan[FO_WAVES];
    const int tid = threadIdx.x;
    int32_t carry = 0;
    for (int32_t tb = 0; tb < p.ntrees; tb += FO_BLOCK) {
        const int32_t t = tb + tid;
        const int32_t v = t < p.ntrees ? 2 * p.nsplit[t] : 0;
        int32_t total;
        const int32_t pref = carry + block_excl_scan<int32_t>(v, &total, s_scan);
        carry += total;
        if (t < p.ntrees) p.tstart_next[t] = pref;
    }
    if (tid == 0) {
        p.tstart_next[p.ntrees] = carry;
        p.rec[0] = carry;
        p.rec[1] = p.rec[2] = p.rec[3] = 0;
    }
}

// ---- stable partition: one wave per open node --------------------------------------------------------------------------------------
__global__ __launch_bounds__(FO_BLOCK) void forest_partition_kernel(Level p, int32_t nopen)
{
    const int lane = threadIdx.x & 63;
    const int64_t oi = (int64_t)blockIdx.x * FO_WAVES + (threadIdx.x >> 6);
    if (oi >= nopen) return;
    const int32_t child = p.dec_child[oi];
    if (child < 0) return;
    const OpenNode nd = p.open[oi];
    const int32_t cnt = nd.end - nd.beg, nl = p.dec_nl[oi], f = p.dec_feat[oi];
    const double thr = p.dec_thr[oi];
    const int32_t *src = p.rows + (int64_t)nd.tree * p.Nb;
    int32_t *dst = p.rows_next + (int64_t)nd.tree * p.Nb;
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
    int32_t nleft = 0, nright = 0;
    for (int32_t j0 = 0; j0 < cnt; j0 += 64) {
        const int32_t j = j0 + lane;
        const bool live = j < cnt;
        const int32_t row = live ? src[nd.beg + j] : 0;
        const bool goes = live && (double)p.xT[(int64_t)f * p.N + row] < thr;
        const uint64_t ml = __ballot(goes), mr = __ballot(live && !goes);
        // (the left part has nl rows by the definition of the boundary; the bound keeps a wrong nl inside the node's segment)
        const int32_t at = nd.beg + (goes ? nleft + __popcll(ml & below) : nl + nright + __popcll(mr & below));
        if (live && at < nd.end) dst[at] = row;
        nleft += __popcll(ml);
        nright += __popcll(mr);
    }
    if (lane == 0) {
        const int32_t slot = p.tstart_next[nd.tree] + p.dec_slot[oi];
        const int32_t mid = nd.beg + nl;
        p.open_next[slot] = OpenNode{nd.tree, child, nd.beg, mid, nd.depth + 1};
        p.open_next[slot + 1] = OpenNode{nd.tree, child + 1, mid, nd.end, nd.depth + 1};
        for (int s = 0; s < 2; ++s) {
            const int32_t c = s == 0 ? nl : cnt - nl;
            const int cls = c <= 64 ? 0 : c <= FO_MID ? 1 : 2;
            const int32_t q = atomicAdd(&p.rec[1 + cls], 1);
            p.lists_next[(int64_t)cls * p.cap + q] = slot + s;
        }
    }
}

// ---- prediction: one thread per (row, tree) ------------------------------------------------------------------------------------------
__global__ void forest_predict_kernel(int64_t count, int32_t ntrees, int32_t n, int32_t k, const float *__restrict__ x,
                                      const int64_t *__restrict__ tree_off, const int32_t *__restrict__ feature,
                                      const double *__restrict__ threshold, const int32_t *__restrict__ left,
                                      const int32_t *__restrict__ right, const int32_t *__restrict__ label, int32_t *__restrict__ votes)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int64_t r = i / ntrees;
    const int64_t b = tree_off[i % ntrees];
    const float *xr = x + r * n;
    int32_t at = 0;
    for (int32_t f = feature[b]; f >= 0; f = feature[b + at]) at = (double)xr[f] < threshold[b + at] ? left[b + at] : right[b + at];
    atomicAdd(&votes[r * k + label[b + at]], 1);  // (integers: the order changes nothing)
}

}  // namespace forest
}  // namespace polee

using namespace polee;
using namespace polee::forest;

struct polee_forest {
    polee_ctx *ctx = nullptr;
    int32_t n = 0, k = 0;
    polee_forest_opts o;
    // the forest, on the host and (CSR, for prediction) on the device
    int32_t ntrees = 0;
    std::vector<int64_t> tree_off;
    std::vector<int32_t> feature, left, right, label;
    std::vector<double> threshold;
    DevBuf<int64_t> d_off;
    DevBuf<int32_t> d_feature, d_left, d_right, d_label, d_votes;
    DevBuf<double> d_threshold;
    // training
    DevBuf<float> d_x, d_xT, d_z0, d_lx;
    DevBuf<uint8_t> d_labels;
    DevBuf<double> d_T, d_dthr, d_bthr;
    DevBuf<int32_t> d_rows[2], d_tstart[2], d_lists[2], d_rec, d_counts, d_dchild, d_dslot, d_dfeat, d_dnl, d_tree_nodes, d_nsplit,
        d_bfeature, d_bleft, d_bright, d_blabel;
    DevBuf<OpenNode> d_open[2];
    DevBuf<Best> d_best;
};

namespace {

polee_status load_nodes(polee_forest *f, int32_t ntrees, const int64_t *off, const int32_t *feature, const double *threshold,
                        const int32_t *left, const int32_t *right, const int32_t *label)
{
    polee_ctx *ctx = f->ctx;
    const size_t nn = (size_t)off[ntrees];
    f->ntrees = ntrees;
    f->tree_off.assign(off, off + ntrees + 1);
    f->feature.assign(feature, feature + nn);
    f->threshold.assign(threshold, threshold + nn);
    f->left.assign(left, left + nn);
    f->right.assign(right, right + nn);
    f->label.assign(label, label + nn);
    POLEE_TRY(f->d_off.upload(ctx, f->tree_off));
    POLEE_TRY(f->d_feature.upload(ctx, f->feature));
    POLEE_TRY(f->d_threshold.upload(ctx, f->threshold));
    POLEE_TRY(f->d_left.upload(ctx, f->left));
    POLEE_TRY(f->d_right.upload(ctx, f->right));
    return f->d_label.upload(ctx, f->label);
}

template <int KP>
void launch_search(const Level &L, const int32_t *rec, hipStream_t st)
{
    if (rec[1] > 0)
        hipLaunchKernelGGL((forest_search_wave_kernel<KP>), dim3((unsigned)ceil_div((int64_t)rec[1] * L.nchunks, FO_WAVES)), dim3(FO_BLOCK), 0,
                           st, L, rec[1]);
    if (rec[2] > 0)
        hipLaunchKernelGGL((forest_search_block_kernel<FO_MID, KP>), dim3((unsigned)((int64_t)rec[2] * L.nchunks)), dim3(FO_BLOCK), 0, st, L,
                           rec[2], 1);
    if (rec[3] > 0)
        hipLaunchKernelGGL((forest_search_block_kernel<POLEE_FOREST_MAX_ROWS, KP>), dim3((unsigned)((int64_t)rec[3] * L.nchunks)),
                           dim3(FO_BLOCK), 0, st, L, rec[3], 2);
}

// grows the forest on d_xT [n][N] / d_labels [N] and loads it into the handle
polee_status grow(polee_forest *f, int64_t N, uint64_t seed)
{
    polee_ctx *ctx = f->ctx;
    hipStream_t st = ctx->stream;
    const polee_forest_opts &o = f->o;
    const int32_t T = o.ntrees, Nb = (int32_t)nboot_of((int32_t)N, o.partial_sampling), maxn = 2 * Nb - 1;
    const int64_t cap = (int64_t)T * Nb;
    if (cap > INT32_MAX / 2) return fail(ctx, POLEE_ERR_UNSUPPORTED, "polee_forest: %d trees of %d rows; the level lists index 2^30 rows", T, Nb);
    std::vector<double> Tab((size_t)Nb + 1);
    clogc_table(Tab.data(), Nb);
    POLEE_TRY(f->d_T.upload(ctx, Tab));
    for (int i = 0; i < 2; ++i) {
        POLEE_TRY(f->d_rows[i].alloc(ctx, (size_t)cap));
        POLEE_TRY(f->d_open[i].alloc(ctx, (size_t)cap));
        POLEE_TRY(f->d_tstart[i].alloc(ctx, (size_t)T + 1));
        POLEE_TRY(f->d_lists[i].alloc(ctx, (size_t)cap * 3));
    }
    POLEE_TRY(f->d_rec.alloc(ctx, 4));
    POLEE_TRY(f->d_counts.alloc(ctx, (size_t)cap * FO_MAX_K));
    POLEE_TRY(f->d_dchild.alloc(ctx, (size_t)cap));
    POLEE_TRY(f->d_dslot.alloc(ctx, (size_t)cap));
    POLEE_TRY(f->d_dfeat.alloc(ctx, (size_t)cap));
    POLEE_TRY(f->d_dnl.alloc(ctx, (size_t)cap));
    POLEE_TRY(f->d_dthr.alloc(ctx, (size_t)cap));
    POLEE_TRY(f->d_tree_nodes.alloc(ctx, (size_t)T));
    POLEE_TRY(f->d_nsplit.alloc(ctx, (size_t)T));
    const size_t padded = (size_t)T * maxn;
    POLEE_TRY(f->d_bfeature.alloc(ctx, padded));
    POLEE_TRY(f->d_bleft.alloc(ctx, padded));
    POLEE_TRY(f->d_bright.alloc(ctx, padded));
    POLEE_TRY(f->d_blabel.alloc(ctx, padded));
    POLEE_TRY(f->d_bthr.alloc(ctx, padded));
    Level L{};
    L.xT = f->d_xT.p;
    L.labels = f->d_labels.p;
    L.T = f->d_T.p;
    L.rec = f->d_rec.p;
    L.counts = f->d_counts.p;
    L.dec_child = f->d_dchild.p;
    L.dec_slot = f->d_dslot.p;
    L.dec_feat = f->d_dfeat.p;
    L.dec_nl = f->d_dnl.p;
    L.dec_thr = f->d_dthr.p;
    L.tree_nodes = f->d_tree_nodes.p;
    L.nsplit = f->d_nsplit.p;
    L.feature = f->d_bfeature.p;
    L.left = f->d_bleft.p;
    L.right = f->d_bright.p;
    L.label = f->d_blabel.p;
    L.threshold = f->d_bthr.p;
    L.N = N;
    L.cap = cap;
    L.seed = seed;
    L.n = f->n;
    L.k = f->k;
    L.Nb = Nb;
    L.ntrees = T;
    L.maxn = maxn;
    L.nsub = nsub_of(f->n, o.nsubfeatures);
    L.max_depth = o.max_depth;
    L.min_leaf = o.min_samples_leaf;
    L.min_split = o.min_samples_split;
    hipLaunchKernelGGL(forest_init_kernel, dim3((unsigned)ceil_div(std::max<int64_t>(cap, T), FO_BLOCK)), dim3(FO_BLOCK), 0, st, L,
                       f->d_rows[0].p, f->d_open[0].p, f->d_tstart[0].p, f->d_lists[0].p, f->d_rec.p);
    POLEE_KERNEL_CHECK(ctx);
    int32_t rec[4];
    POLEE_TRY(f->d_rec.download(ctx, rec, 4));
    for (int level = 0, cur = 0; rec[0] > 0; ++level, cur ^= 1) {
        if (level > maxn) return fail(ctx, POLEE_ERR_HIP, "polee_forest: the level loop did not end");
        const int32_t nopen = rec[0];
        if (nopen > cap || rec[1] + rec[2] + rec[3] != nopen) return fail(ctx, POLEE_ERR_HIP, "polee_forest: inconsistent level record");
        // few open nodes: the candidates are cut into more chunks, so that the level still fills the machine
        int64_t nchunks = std::min<int64_t>(std::max<int64_t>(1, FO_TARGET_ITEMS / nopen), ceil_div(L.nsub, FO_MIN_CHUNK));
        L.csize = (int32_t)ceil_div(L.nsub, nchunks);
        L.nchunks = (int32_t)ceil_div(L.nsub, L.csize);
        POLEE_TRY(f->d_best.alloc(ctx, (size_t)nopen * L.nchunks));
        L.best = f->d_best.p;
        L.rows = f->d_rows[cur].p;
        L.rows_next = f->d_rows[cur ^ 1].p;
        L.open = f->d_open[cur].p;
        L.open_next = f->d_open[cur ^ 1].p;
        L.tstart = f->d_tstart[cur].p;
        L.tstart_next = f->d_tstart[cur ^ 1].p;
        L.lists = f->d_lists[cur].p;
        L.lists_next = f->d_lists[cur ^ 1].p;
        if (f->k <= 4)
            launch_search<4>(L, rec, st);
        else
            launch_search<16>(L, rec, st);
        hipLaunchKernelGGL(forest_pick_kernel, dim3((unsigned)T), dim3(FO_BLOCK), 0, st, L);
        hipLaunchKernelGGL(forest_level_scan_kernel, dim3(1), dim3(FO_BLOCK), 0, st, L);
        hipLaunchKernelGGL(forest_partition_kernel, dim3((unsigned)ceil_div(nopen, FO_WAVES)), dim3(FO_BLOCK), 0, st, L, nopen);
        POLEE_KERNEL_CHECK(ctx);
        POLEE_TRY(f->d_rec.download(ctx, rec, 4));
    }
    // the padded per-tree arrays -> CSR
    std::vector<int32_t> counts((size_t)T), pf(padded), pl(padded), pr(padded), pb(padded);
    std::vector<double> pt(padded);
    POLEE_TRY(f->d_tree_nodes.download(ctx, counts.data(), (size_t)T));
    POLEE_TRY(f->d_bfeature.download(ctx, pf.data(), padded));
    POLEE_TRY(f->d_bleft.download(ctx, pl.data(), padded));
    POLEE_TRY(f->d_bright.download(ctx, pr.data(), padded));
    POLEE_TRY(f->d_blabel.download(ctx, pb.data(), padded));
    POLEE_TRY(f->d_bthr.download(ctx, pt.data(), padded));
    std::vector<int64_t> off((size_t)T + 1, 0);
    for (int32_t t = 0; t < T; ++t) {
        if (counts[(size_t)t] < 1 || counts[(size_t)t] > maxn) return fail(ctx, POLEE_ERR_HIP, "polee_forest: tree %d has %d nodes", t, counts[(size_t)t]);
        off[(size_t)t + 1] = off[(size_t)t] + counts[(size_t)t];
    }
    const size_t nn = (size_t)off[(size_t)T];
    std::vector<int32_t> cf(nn), cl(nn), cr(nn), cb(nn);
    std::vector<double> ct(nn);
    for (int32_t t = 0; t < T; ++t) {
        const size_t s = (size_t)t * maxn, d = (size_t)off[(size_t)t], c = (size_t)counts[(size_t)t];
        std::copy(pf.begin() + s, pf.begin() + s + c, cf.begin() + d);
        std::copy(pl.begin() + s, pl.begin() + s + c, cl.begin() + d);
        std::copy(pr.begin() + s, pr.begin() + s + c, cr.begin() + d);
        std::copy(pb.begin() + s, pb.begin() + s + c, cb.begin() + d);
        std::copy(pt.begin() + s, pt.begin() + s + c, ct.begin() + d);
    }
    int32_t bt = 0;
    int64_t bn = 0;
    if (!nodes_ok(f->n, f->k, T, off.data(), cf.data(), cl.data(), cr.data(), cb.data(), &bt, &bn))
        return fail(ctx, POLEE_ERR_HIP, "polee_forest: the builder left a malformed node %lld in tree %d", (long long)bn, bt);
    return load_nodes(f, T, off.data(), cf.data(), ct.data(), cl.data(), cr.data(), cb.data());
}

polee_status upload_labels(polee_forest *f, const int32_t *labels, int64_t count, int32_t repeat)
{
    polee_ctx *ctx = f->ctx;
    std::vector<uint8_t> lab((size_t)count * repeat);
    for (int64_t i = 0; i < count; ++i) {
        if (labels[i] < 0 || labels[i] >= f->k) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_forest: label %d of row %lld", labels[i], (long long)i);
        for (int32_t d = 0; d < repeat; ++d) lab[(size_t)d * count + i] = (uint8_t)labels[i];
    }
    return f->d_labels.upload(ctx, lab);
}

polee_status check_rows(polee_forest *f, int64_t N)
{
    polee_ctx *ctx = f->ctx;
    if (N < 1 || N >= FO_MAX_N_ROWS) return fail(ctx, POLEE_ERR_UNSUPPORTED, "polee_forest: %lld training rows", (long long)N);
    const int64_t Nb = nboot_of((int32_t)N, f->o.partial_sampling);
    if (Nb > POLEE_FOREST_MAX_ROWS)
        return fail(ctx, POLEE_ERR_UNSUPPORTED, "polee_forest: %lld rows per tree; the builders take up to %d (lower partial_sampling)",
                    (long long)Nb, POLEE_FOREST_MAX_ROWS);
    return POLEE_OK;
}

void launch_layout(polee_forest *f, const float *d_in, int32_t R, int take_log, int64_t N, int64_t r0)
{
    hipLaunchKernelGGL(forest_layout_kernel, dim3((unsigned)ceil_div(f->n, 32), (unsigned)ceil_div(R, 32)), dim3(256), 0, f->ctx->stream, d_in,
                       R, f->n, take_log, f->d_xT.p, N, r0);
}

polee_status predict_rows(polee_forest *f, const float *d_x, int32_t R)
{
    polee_ctx *ctx = f->ctx;
    const int64_t count = (int64_t)R * f->ntrees;
    hipLaunchKernelGGL(forest_predict_kernel, dim3((unsigned)ceil_div(count, FO_BLOCK)), dim3(FO_BLOCK), 0, ctx->stream, count, f->ntrees,
                       f->n, f->k, d_x, (const int64_t *)f->d_off.p, (const int32_t *)f->d_feature.p, (const double *)f->d_threshold.p,
                       (const int32_t *)f->d_left.p, (const int32_t *)f->d_right.p, (const int32_t *)f->d_label.p, f->d_votes.p);
    POLEE_KERNEL_CHECK(ctx);
    return POLEE_OK;
}

}  // namespace

extern "C" {

polee_status polee_forest_create(polee_ctx *ctx, int32_t n, int32_t k, const polee_forest_opts *opts, polee_forest **out)
{
    return ctx_entry(ctx, "polee_forest_create", [&]() -> polee_status {
        if (!out || n < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_forest_create: bad argument");
        if (k < 2 || k > FO_MAX_K) return fail(ctx, POLEE_ERR_UNSUPPORTED, "polee_forest_create: %d classes; the kernels are built for 2..16", k);
        polee_forest_opts o;
        polee_forest_default_opts(&o);
        if (opts) o = *opts;
        if (const char *why = check_opts(o, n, k)) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_forest_create: %s", why);
        polee_forest *f = new polee_forest();
        f->ctx = ctx;
        ctx_retain(ctx);
        f->n = n;
        f->k = k;
        f->o = o;
        *out = f;
        return POLEE_OK;
    });
}

void polee_forest_destroy(polee_forest *f)
{
    if (!f) return;
    polee_ctx *ctx = f->ctx;
    if (ctx) (void)hipSetDevice(ctx->device);
    delete f;
    ctx_release(ctx);
}

polee_status polee_forest_fit_points(polee_forest *f, const float *x, const int32_t *labels, int32_t N, uint64_t seed)
{
    return entry(f, "polee_forest_fit_points", [&](polee_ctx *ctx) -> polee_status {
        if (!labels) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_forest_fit_points: null argument");
        POLEE_TRY(check_points(ctx, "polee_forest", x, N, f->n));
        POLEE_TRY(check_rows(f, N));
        POLEE_TRY(upload_labels(f, labels, N, 1));
        POLEE_TRY(f->d_x.upload(ctx, x, (size_t)N * f->n));
        POLEE_TRY(f->d_xT.alloc(ctx, (size_t)N * f->n));
        launch_layout(f, f->d_x.p, N, 0, N, 0);
        POLEE_KERNEL_CHECK(ctx);
        return grow(f, N, seed);
    });
}

polee_status polee_forest_fit(polee_forest *f, polee_approx *ap, const int32_t *labels, int32_t ndraws, uint64_t draw_seed, uint64_t seed,
                              const float *z0)
{
    return entry(f, "polee_forest_fit", [&](polee_ctx *ctx) -> polee_status {
        int32_t S = 0;
        POLEE_TRY(check_approx(ctx, "polee_forest", ap, f->n, 0, &S));
        if (!labels || ndraws < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_forest_fit: bad argument");
        const int64_t N = (int64_t)ndraws * S;
        POLEE_TRY(check_rows(f, N));
        POLEE_TRY(upload_labels(f, labels, S, ndraws));
        DrawFeed feed(ap, f->d_z0, S, f->n, draw_seed);
        const float *d_x = nullptr;
        POLEE_TRY(feed.upload(z0, (size_t)ndraws));
        POLEE_TRY(f->d_xT.alloc(ctx, (size_t)N * f->n));
        for (int32_t d = 0; d < ndraws; ++d) {
            POLEE_TRY(feed.draw((uint64_t)d, (size_t)d, &d_x));
            launch_layout(f, d_x, S, 1, N, (int64_t)d * S);
            POLEE_KERNEL_CHECK(ctx);
        }
        return grow(f, N, seed);
    });
}

polee_status polee_forest_node_count(polee_forest *f, int32_t *ntrees, int64_t *nnodes)
{
    return entry(f, "polee_forest_node_count", [&](polee_ctx *ctx) -> polee_status {
        if (!ntrees || !nnodes) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_forest_node_count: null argument");
        *ntrees = f->ntrees;
        *nnodes = f->ntrees ? f->tree_off[(size_t)f->ntrees] : 0;
        return POLEE_OK;
    });
}

polee_status polee_forest_get_nodes(polee_forest *f, int64_t *tree_off, int32_t *feature, double *threshold, int32_t *left, int32_t *right,
                                    int32_t *label)
{
    return entry(f, "polee_forest_get_nodes", [&](polee_ctx *ctx) -> polee_status {
        if (!tree_off || !feature || !threshold || !left || !right || !label)
            return fail(ctx, POLEE_ERR_BAD_ARG, "polee_forest_get_nodes: null argument");
        if (!f->ntrees) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_forest_get_nodes: no forest yet");
        std::copy(f->tree_off.begin(), f->tree_off.end(), tree_off);
        std::copy(f->feature.begin(), f->feature.end(), feature);
        std::copy(f->threshold.begin(), f->threshold.end(), threshold);
        std::copy(f->left.begin(), f->left.end(), left);
        std::copy(f->right.begin(), f->right.end(), right);
        std::copy(f->label.begin(), f->label.end(), label);
        return POLEE_OK;
    });
}

polee_status polee_forest_set_nodes(polee_forest *f, int32_t ntrees, const int64_t *tree_off, const int32_t *feature,
                                    const double *threshold, const int32_t *left, const int32_t *right, const int32_t *label)
{
    return entry(f, "polee_forest_set_nodes", [&](polee_ctx *ctx) -> polee_status {
        if (ntrees < 1 || ntrees > FO_MAX_TREES || !tree_off || !feature || !threshold || !left || !right || !label)
            return fail(ctx, POLEE_ERR_BAD_ARG, "polee_forest_set_nodes: bad argument");
        int32_t bt = 0;
        int64_t bn = 0;
        if (!nodes_ok(f->n, f->k, ntrees, tree_off, feature, left, right, label, &bt, &bn))
            return fail(ctx, POLEE_ERR_BAD_ARG, "polee_forest_set_nodes: node %lld of tree %d is malformed", (long long)bn, bt);
        return load_nodes(f, ntrees, tree_off, feature, threshold, left, right, label);
    });
}

polee_status polee_forest_predict_points(polee_forest *f, const float *x, int32_t R, int32_t *votes)
{
    return entry(f, "polee_forest_predict_points", [&](polee_ctx *ctx) -> polee_status {
        if (!votes) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_forest_predict_points: null argument");
        if (!f->ntrees) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_forest_predict_points: no forest yet");
        POLEE_TRY(check_points(ctx, "polee_forest", x, R, f->n));
        POLEE_TRY(f->d_x.upload(ctx, x, (size_t)R * f->n));
        POLEE_TRY(f->d_votes.alloc(ctx, (size_t)R * f->k));
        POLEE_HIP_TRY(ctx, hipMemsetAsync(f->d_votes.p, 0, (size_t)R * f->k * sizeof(int32_t), ctx->stream));
        POLEE_TRY(predict_rows(f, f->d_x.p, R));
        return f->d_votes.download(ctx, votes, (size_t)R * f->k);
    });
}

polee_status polee_forest_predict(polee_forest *f, polee_approx *ap, int32_t ndraws, uint64_t seed, const float *z0, int32_t *votes)
{
    return entry(f, "polee_forest_predict", [&](polee_ctx *ctx) -> polee_status {
        int32_t S = 0;
        POLEE_TRY(check_approx(ctx, "polee_forest", ap, f->n, 0, &S));
        if (!votes || ndraws < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_forest_predict: bad argument");
        if (!f->ntrees) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_forest_predict: no forest yet");
        const size_t sn = (size_t)S * f->n;
        DrawFeed feed(ap, f->d_z0, S, f->n, seed);
        const float *d_x = nullptr;
        POLEE_TRY(feed.upload(z0, (size_t)ndraws));
        POLEE_TRY(f->d_lx.alloc(ctx, sn));
        POLEE_TRY(f->d_votes.alloc(ctx, (size_t)S * f->k));
        POLEE_HIP_TRY(ctx, hipMemsetAsync(f->d_votes.p, 0, (size_t)S * f->k * sizeof(int32_t), ctx->stream));
        for (int32_t d = 0; d < ndraws; ++d) {
            POLEE_TRY(feed.draw((uint64_t)d, (size_t)d, &d_x));
            hipLaunchKernelGGL(forest_log_kernel, dim3((unsigned)ceil_div((int64_t)sn, FO_BLOCK)), dim3(FO_BLOCK), 0, ctx->stream, (int64_t)sn,
                               d_x, f->d_lx.p);
            POLEE_TRY(predict_rows(f, f->d_lx.p, S));
        }
        return f->d_votes.download(ctx, votes, (size_t)S * f->k);
    });
}

polee_status polee_forest_log_draws(polee_approx *ap, int32_t ndraws, uint64_t seed, const float *z0, float *out)
{
    return entry(ap, "polee_forest_log_draws", [&](polee_ctx *ctx) -> polee_status {
        int32_t S = 0, n = 0;
        approx_dims(ap, &S, &n);
        if (!out || ndraws < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_forest_log_draws: bad argument");
        const size_t sn = (size_t)S * n;
        DevBuf<float> d_z0, d_lx;
        DrawFeed feed(ap, d_z0, S, n, seed);
        const float *d_x = nullptr;
        POLEE_TRY(feed.upload(z0, (size_t)ndraws));
        POLEE_TRY(d_lx.alloc(ctx, sn));
        for (int32_t d = 0; d < ndraws; ++d) {
            POLEE_TRY(feed.draw((uint64_t)d, (size_t)d, &d_x));
            hipLaunchKernelGGL(forest_log_kernel, dim3((unsigned)ceil_div((int64_t)sn, FO_BLOCK)), dim3(FO_BLOCK), 0, ctx->stream, (int64_t)sn,
                               d_x, d_lx.p);
            POLEE_KERNEL_CHECK(ctx);
            POLEE_TRY(d_lx.download(ctx, out + (size_t)d * sn, sn));
        }
        return POLEE_OK;
    });
}

}  // extern "C"
