// `polee model tsne` (models/tsne.jl:52-99, models/polee_tsne.py:17-185, :213-398 with use_vlr=True, alpha=1, no neural network):
// parametric t-SNE of log expression.  Every step draws one sample from each of the S fitted approximations, measures the batch rows'
// pairwise distance over all n transcripts and takes one Adam step on the linear embedding z = lx W.  DESIGN.md section 3.13.
//
//   lx        = log of a draw [S][n], or the uploaded points (log expression already)
//   z         = lx W                                   W [n][C], C <= 16; the bias b stays at zero (decision 2 below)
//   delta_ab  = sum_j (lx_aj - lx_bj)^2 / n - (mean_a - mean_b)^2      the variance of the log-ratio ("VLR"); use_vlr = 0: the plain
//               sum of squares                                          (pairwise_vlr :17-26, pairwise_l2_sq :42-48)
//   P on the batch I (B indices, in order), Q on all S samples, loss = sum_{a,b in I} P_ab log(P_ab / Q_ab)   (:136-185, :337)
//
// Per step, on the context's stream, nothing waits for the device:
//   1. approx_sample_device        the draw x [S][n] (approx.hip), clipped at 1e-16 so logf is finite
//   2. tsne_project_kernel         chunk_project (draw_model.hpp) without a bias: besides the C partial sums of z it writes the
//                                  chunk's sum of lx (the row means cost no read of their own); partials [chunks][S][C] and [chunks][S]
//   3. tsne_finish_kernel          one workgroup per sample: the partials summed in f64 in a fixed order -> z f64 [S][C], the row
//                                  mean in f64, its f32 rounding mhat and the residue mean - mhat; the sample's position in I
//   4. tsne_pairwise_kernel        THE HOT PATH.  A workgroup takes one pair of 64-row tiles of the batch and TS_CHUNK transcripts;
//                                  it stages lx - mhat of 64 transcripts x 64 rows per tile in LDS (the log is taken once per
//                                  staged value, not once per pair) and every thread keeps a 4 x 4 block of pair sums
//                                  sum_j (c_aj - c_bj)^2 in f32 registers; partials [tile pairs][chunks][64][64]
//   5. tsne_delta_kernel           the chunk partials of a pair summed in f64 in a fixed order, / n, minus the squared difference of
//                                  the two residues (exact: the centred values' own mean); written to [a][b] and [b][a], diagonal 0
//   6. tsne_sums_kernel            column sums of E on the batch, row sums of the Student kernel k on all samples
//   7. tsne_loss_kernel            per batch row: P, Q, R = P / Q, the row's loss and its share of sum R o Q
//   8. tsne_dz_kernel              per sample: dz_i = 2 sum_j A_ij (z_i - z_j); workgroup 0 writes the step's loss
//   9. tsne_grad_update_kernel     grad_accumulate, one thread per transcript: g_W[j][c] = sum_s lx[s][j] dz[s][c], then Adam
//                                  (tf_adam) on W in the same thread; in evaluation mode the gradient is handed out instead
// Steps 6 - 8 are f64 throughout.  There are no float atomics and every sum has a fixed order: results are bitwise reproducible.
// The projection, the gradient accumulation, the f64 sums, Adam and the draw loop are draw_model.hpp's, shared with classify.hip.
// The centred form is used, not the Gram form r_a + r_b - 2 x_a.x_b: replicate samples have a delta two orders of magnitude below
// r / n, so the Gram form cancels, and on gfx950 the f32-input matrix instructions run at the f32 vector rate anyway.
//
// Where the reference is broken or ill-defined:
//   1. polee_tsne.py:222-230 calls the sampler with a stale signature and cannot run as written; its intent, one draw per sample
//      per evaluation with no gradient through it, is what is built.
//   2. The loss depends on z through differences only, so the exact gradient of the bias b is zero and Adam on its rounding noise
//      would random-walk b by +-lr per step: b is kept at zero and not trained.  The embedding is the reference's up to a
//      translation below num_steps lr.
//   3. --posterior-mean is parsed by the reference and never read; here it selects the point path (the *_points entries): x is the
//      fixed log of the samples' posterior mean, no draws.
//   4. W0 and the minibatches come from the host (polee_amd/tsne.py: NumPy generators keyed by the seed); draw index i (DrawFeed)
//      is -1 for the bandwidth draw, t - 1 for Adam step t, T .. T+9 for the embedding after T steps.
// Parameters and moments are stored transposed, wT [C][n] (the ABI speaks W [n][C]).
#include "draw_model.hpp"

namespace polee {

constexpr int TS_ROWS = 64;     // rows of a tile of the pairwise kernel
constexpr int TS_SUB = 64;      // transcripts staged in LDS at a time
constexpr int TS_SUBP = TS_SUB + 1;  // (an odd row pitch: the 16 rows a half-wave reads sit in 16 banks)
constexpr int TS_CHUNK = 512;   // transcripts per workgroup of the pairwise kernel: the length of an f32 chain

// tile pair number -> (ti, tj), ti <= tj < T, in the order (0,0) (0,1) .. (0,T-1) (1,1) ..
__device__ inline void tile_pair(int tp, int T, int &ti, int &tj)
{
    ti = 0;
    while (tp >= T - ti) {
        tp -= T - ti;
        ++ti;
    }
    tj = ti + tp;
}

// part [nchunks][S][C], rpart [nchunks][S]: the chunk's sum of lx
template <int KP>
__global__ __launch_bounds__(DM_BLOCK) void tsne_project_kernel(int n, int S, int C, int nchunks, const float *__restrict__ x, int is_log,
                                                               const float *__restrict__ W, float *__restrict__ part,
                                                               float *__restrict__ rpart)
{
    chunk_project<KP, false, true>(n, S, C, nchunks, x, is_log, W, nullptr, part, nullptr, rpart);
}

// grid S.  z f64 [S][C]; zacc (or null) += z; mean - mhat -> resid, mhat (both 0 without use_vlr); pos[s] = the position of s in
// idx [B], -1 when it is not in the batch (idx null: not written)
template <int KP>
__global__ __launch_bounds__(DM_BLOCK) void tsne_finish_kernel(int n, int S, int C, int nchunks, int use_vlr,
                                                              const float *__restrict__ part, const float *__restrict__ rpart,
                                                              const int32_t *__restrict__ idx, int B, double *__restrict__ z,
                                                              double *__restrict__ zacc, float *__restrict__ mhat,
                                                              double *__restrict__ resid, int32_t *__restrict__ pos)
{
    __shared__ double red[DM_BLOCK];
    __shared__ int spos;
    const int tid = threadIdx.x, s = blockIdx.x;
    double r = 0.0;
    for (int ch = tid; ch < nchunks; ch += DM_BLOCK) r += (double)rpart[(int64_t)ch * S + s];
    r = block_sum(r, red);
    if (tid == 0) {
        const double mean = use_vlr ? r / (double)n : 0.0;
        const float mh = (float)mean;
        mhat[s] = mh;
        resid[s] = mean - (double)mh;
        spos = -1;
    }
    chunk_sum<KP, true>(part, S, C, nchunks, s, red);
    if (tid < C) {
        z[(int64_t)s * C + tid] = red[tid];
        if (zacc) zacc[(int64_t)s * C + tid] += red[tid];
    }
    if (!idx) return;  // (uniform)
    for (int b = tid; b < B; b += DM_BLOCK)
        if (idx[b] == s) spos = b;  // (at most one: the batch has no repeated index)
    __syncthreads();
    if (tid == 0) pos[s] = spos;
}

// grid ntp * nchunks, workgroup tp * nchunks + chunk.  part [ntp][nchunks][64][64]: sum over the chunk's transcripts of
// (c_a - c_b)^2, c = lx - mhat, for local rows a of tile ti and b of tile tj (rows past B and transcripts past n are staged as 0)
__global__ __launch_bounds__(DM_BLOCK) void tsne_pairwise_kernel(int n, int B, int nchunks, const float *__restrict__ x, int is_log,
                                                                const int32_t *__restrict__ idx, const float *__restrict__ mhat,
                                                                float *__restrict__ part)
{
    __shared__ float sA[TS_ROWS * TS_SUBP];
    __shared__ float sB[TS_ROWS * TS_SUBP];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int chunk = blockIdx.x % nchunks;
    int ti, tj;
    tile_pair(blockIdx.x / nchunks, (B + TS_ROWS - 1) / TS_ROWS, ti, tj);
    const bool diag = ti == tj;
    const float *sb = diag ? sA : sB;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[i][k] = 0.0f;
    const int64_t jbeg = (int64_t)chunk * TS_CHUNK;
    const int64_t jend = jbeg + TS_CHUNK < n ? jbeg + TS_CHUNK : n;
    for (int64_t j0 = jbeg; j0 < jend; j0 += TS_SUB) {
        __syncthreads();
        for (int e = tid; e < TS_ROWS * TS_SUB; e += DM_BLOCK) {  // (a wave: 64 consecutive transcripts of one row)
            const int r = e >> 6, jj = e & 63;
            const int64_t j = j0 + jj;
            const int pa = ti * TS_ROWS + r, pb = tj * TS_ROWS + r;
            float va = 0.0f, vb = 0.0f;
            if (j < jend && pa < B) {
                const int sa = idx[pa];
                const float v = x[(int64_t)sa * n + j];
                va = (is_log ? v : logf(v)) - mhat[sa];
            }
            sA[r * TS_SUBP + jj] = va;
            if (!diag) {
                if (j < jend && pb < B) {
                    const int sbi = idx[pb];
                    const float v = x[(int64_t)sbi * n + j];
                    vb = (is_log ? v : logf(v)) - mhat[sbi];
                }
                sB[r * TS_SUBP + jj] = vb;
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int jj = 0; jj < TS_SUB; ++jj) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[i] = sA[(ty + 16 * i) * TS_SUBP + jj];
                b[i] = sb[(tx + 16 * i) * TS_SUBP + jj];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float d = a[i] - b[k];
                    acc[i][k] = fmaf(d, d, acc[i][k]);
                }
        }
    }
    float *out = part + (int64_t)blockIdx.x * (TS_ROWS * TS_ROWS);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) out[(ty + 16 * i) * TS_ROWS + tx + 16 * k] = acc[i][k];
}

// grid ntp * 64, workgroup tp * 64 + local row a; thread (stripe q, local row b).  delta f64 [B][B], exactly symmetric, diagonal 0
__global__ __launch_bounds__(DM_BLOCK) void tsne_delta_kernel(int n, int B, int nchunks, int use_vlr, const float *__restrict__ part,
                                                             const int32_t *__restrict__ idx, const double *__restrict__ resid,
                                                             double *__restrict__ delta)
{
    __shared__ double red[DM_BLOCK];
    const int tid = threadIdx.x, rb = tid & 63, q = tid >> 6;
    const int ra = blockIdx.x % TS_ROWS;
    const int tp = blockIdx.x / TS_ROWS;
    int ti, tj;
    tile_pair(tp, (B + TS_ROWS - 1) / TS_ROWS, ti, tj);
    const int pa = ti * TS_ROWS + ra, pb = tj * TS_ROWS + rb;
    if (pa >= B) return;  // (uniform)
    const float *src = part + (int64_t)tp * nchunks * (TS_ROWS * TS_ROWS) + ra * TS_ROWS + rb;
    double a = 0.0;
#pragma unroll 4
    for (int ch = q; ch < nchunks; ch += DM_BLOCK / 64) a += (double)src[(int64_t)ch * (TS_ROWS * TS_ROWS)];
    red[tid] = a;
    __syncthreads();
    if (q != 0 || pb >= B || pa > pb) return;
    if (pa == pb) {
        delta[(int64_t)pa * B + pa] = 0.0;
        return;
    }
    double v = ((red[rb] + red[rb + 64]) + red[rb + 128]) + red[rb + 192];
    if (use_vlr) {
        const double dr = resid[idx[pa]] - resid[idx[pb]];
        v = fmax(v / (double)n - dr * dr, 0.0);
    }
    delta[(int64_t)pa * B + pb] = v;
    delta[(int64_t)pb * B + pa] = v;
}

__device__ inline double tsne_E(double delta, double sigma)
{
    return fmin(fmax(exp(-delta / (2.0 * sigma * sigma)), 1e-12), 1.0);  // (tf.clip_by_value, polee_tsne.py:145-146)
}

__device__ inline double tsne_D(const double *__restrict__ z, int C, int i, int j)
{
    double D = 0.0;
    for (int c = 0; c < C; ++c) {
        const double d = z[(int64_t)i * C + c] - z[(int64_t)j * C + c];
        D += d * d;
    }
    return D;
}

// grid B + S.  Workgroup b < B: cs[b] = sum_{a != b} E_ab, E_ab = clip(exp(-delta_ab / (2 sigma_b^2))): the divisor is the column's
// (polee_tsne.py:145, :151).  Workgroup B + i: rowk[i] = sum_{j != i} (1 + D_ij / alpha)^(-(alpha + 1) / 2)   (:177-182)
__global__ __launch_bounds__(DM_BLOCK) void tsne_sums_kernel(int S, int B, int C, double alpha, const double *__restrict__ delta,
                                                            const int32_t *__restrict__ idx, const float *__restrict__ sigma,
                                                            const double *__restrict__ z, double *__restrict__ cs,
                                                            double *__restrict__ rowk)
{
    __shared__ double red[DM_BLOCK];
    const int tid = threadIdx.x;
    double a = 0.0;
    if ((int)blockIdx.x < B) {
        const int b = blockIdx.x;
        const double sg = (double)sigma[idx[b]];
        for (int r = tid; r < B; r += DM_BLOCK)
            if (r != b) a += tsne_E(delta[(int64_t)r * B + b], sg);
        a = block_sum(a, red);
        if (tid == 0) cs[b] = a;
    } else {
        const int i = blockIdx.x - B;
        for (int j = tid; j < S; j += DM_BLOCK)
            if (j != i) a += pow(1.0 + tsne_D(z, C, i, j) / alpha, -0.5 * (alpha + 1.0));
        a = block_sum(a, red);
        if (tid == 0) rowk[i] = a;
    }
}

// grid B, workgroup = batch row a.  P_ab = (E_ab / cs_b + E_ba / cs_a) / (2 S) + eps (S, not B: polee_tsne.py:166), Q_ab = k_ab / Z
// + eps with Z over ALL samples; R [B][B] = P / Q; lossrow[a] = sum_b P log(P / Q); trow[a] = sum_b R_ab k_ab / Z; Zout[0] = Z
__global__ __launch_bounds__(DM_BLOCK) void tsne_loss_kernel(int S, int B, int C, double alpha, double eps,
                                                            const double *__restrict__ delta, const int32_t *__restrict__ idx,
                                                            const float *__restrict__ sigma, const double *__restrict__ z,
                                                            const double *__restrict__ cs, const double *__restrict__ rowk,
                                                            double *__restrict__ R, double *__restrict__ lossrow,
                                                            double *__restrict__ trow, double *__restrict__ Zout)
{
    __shared__ double red[DM_BLOCK];
    const int tid = threadIdx.x, a = blockIdx.x;
    double zs = 0.0;
    for (int i = tid; i < S; i += DM_BLOCK) zs += rowk[i];
    const double Z = block_sum(zs, red);
    const int ia = idx[a];
    const double sga = (double)sigma[ia], csa = cs[a];
    double L = 0.0, T = 0.0;
    for (int b = tid; b < B; b += DM_BLOCK) {
        const int ib = idx[b];
        double p = 0.0, qv = 0.0;
        if (b != a) {
            const double d = delta[(int64_t)a * B + b];
            p = (tsne_E(d, (double)sigma[ib]) / cs[b] + tsne_E(d, sga) / csa) / (2.0 * (double)S);
            qv = pow(1.0 + tsne_D(z, C, ia, ib) / alpha, -0.5 * (alpha + 1.0)) / Z;
        }
        const double pe = p + eps, qe = qv + eps;
        const double r = pe / qe;
        R[(int64_t)a * B + b] = r;
        L += pe * log(r);
        T += r * qv;
    }
    L = block_sum(L, red);
    T = block_sum(T, red);
    if (tid == 0) {
        lossrow[a] = L;
        trow[a] = T;
        if (a == 0) Zout[0] = Z;
    }
}

// grid S, workgroup = sample i.  dL/dk_ij = -R_ij / Z + T / Z (R = 0 outside I x I, T = sum R o Q without epsilon),
// dk/dD = -((alpha + 1) / (2 alpha)) (1 + D / alpha)^(-(alpha + 3) / 2), dz_i = 2 sum_j (dL/dD_ij + dL/dD_ji) (z_i - z_j).
// Samples outside the batch get their gradient through Z.  Workgroup 0 writes the step's loss.
template <int KP>
__global__ __launch_bounds__(DM_BLOCK) void tsne_dz_kernel(int S, int B, int C, double alpha, const double *__restrict__ z,
                                                          const int32_t *__restrict__ pos, const double *__restrict__ R,
                                                          const double *__restrict__ lossrow, const double *__restrict__ trow,
                                                          const double *__restrict__ Zin, float *__restrict__ dz,
                                                          float *__restrict__ loss_out)
{
    __shared__ double red[DM_BLOCK];
    const int tid = threadIdx.x, i = blockIdx.x;
    double ts = 0.0, ls = 0.0;
    for (int a = tid; a < B; a += DM_BLOCK) {
        ts += trow[a];
        ls += lossrow[a];
    }
    const double T = block_sum(ts, red);
    if (i == 0) {  // (uniform)
        ls = block_sum(ls, red);
        if (tid == 0) loss_out[0] = (float)ls;
    }
    const double Z = Zin[0];
    const int pi = pos[i];
    double zi[KP], acc[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        zi[c] = c < C ? z[(int64_t)i * C + c] : 0.0;
        acc[c] = 0.0;
    }
    for (int j = tid; j < S; j += DM_BLOCK) {
        if (j == i) continue;
        double d[KP], D = 0.0;
#pragma unroll
        for (int c = 0; c < KP; ++c) {
            d[c] = c < C ? zi[c] - z[(int64_t)j * C + c] : 0.0;
            D += d[c] * d[c];
        }
        const int pj = pos[j];
        const double rs = (pi >= 0 && pj >= 0) ? R[(int64_t)pi * B + pj] + R[(int64_t)pj * B + pi] : 0.0;
        const double kd = -((alpha + 1.0) / (2.0 * alpha)) * pow(1.0 + D / alpha, -0.5 * (alpha + 3.0));
        const double A = kd * (2.0 * T - rs) / Z;
#pragma unroll
        for (int c = 0; c < KP; ++c) acc[c] += A * d[c];
    }
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        if (c < C) {  // (uniform)
            const double g = block_sum(acc[c], red);
            if (tid == 0) dz[(int64_t)i * C + c] = (float)(2.0 * g);
        }
    }
}

// One thread per transcript: g[c] = sum_s lx[s][j] dz[s][c].  mode 0: Adam (tf.train.AdamOptimizer, polee_tsne.py:344-345);
// mode 1: g to gout, nothing is updated.  P, M, V, gout: [C][n]
template <int KP>
__global__ __launch_bounds__(DM_BLOCK) void tsne_grad_update_kernel(int n, int S, int C, const float *__restrict__ x, int is_log,
                                                                   const float *__restrict__ dz, float *__restrict__ P,
                                                                   float *__restrict__ M, float *__restrict__ V, float lr_t, float b1,
                                                                   float b2, float eps, int mode, float *__restrict__ gout)
{
    __shared__ float sdz[DM_TILE_S * KP];
    const int tid = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * DM_BLOCK + tid;
    const bool active = j < n;
    float acc[KP];
    double unused;
    grad_accumulate<KP, false, false>(n, S, C, x, is_log, dz, j, active, 0.0f, sdz, acc, unused);
    if (!active) return;
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        if (c >= C) continue;
        const int64_t i = (int64_t)c * n + j;
        const float g = acc[c];
        if (mode == 1) {
            gout[i] = g;
            continue;
        }
        P[i] = tf_adam(P[i], &M[i], &V[i], g, lr_t, b1, b2, eps);
    }
}

}  // namespace polee

using namespace polee;

struct polee_tsne {
    polee_ctx *ctx = nullptr;
    int32_t n = 0, S = 0, C = 0, KP = 0, nchunks = 0;
    int64_t cn = 0;
    int64_t t = 0;  // Adam steps taken: the step clock, which runs on across fit calls
    bool have_sigmas = false;
    polee_tsne_opts o;
    DevBuf<float> d_W, d_M, d_V, d_gout, d_part, d_rpart, d_mhat, d_sigma, d_dz, d_zout, d_loss, d_x, d_z0;
    DevBuf<double> d_z, d_zacc, d_resid, d_rowk, d_Z;
    DevBuf<int32_t> d_pos, d_idx;
    // per batch size (grown on demand)
    DevBuf<float> d_pw;
    DevBuf<double> d_delta, d_R, d_cs, d_lossrow, d_trow;
};

namespace {

int64_t tile_pairs(int32_t B)
{
    const int64_t T = ceil_div(B, TS_ROWS);
    return T * (T + 1) / 2;
}

polee_status check_opts(polee_ctx *ctx, const polee_tsne_opts &o)
{
    if (!(o.alpha > 0.0f) || !std::isfinite(o.alpha) || !(o.eps >= 0.0f) || !std::isfinite(o.eps) || !(o.learning_rate > 0.0f) ||
        !std::isfinite(o.learning_rate) || !(o.beta1 >= 0.0f && o.beta1 < 1.0f) || !(o.beta2 >= 0.0f && o.beta2 < 1.0f) ||
        !(o.epsilon > 0.0f) || !std::isfinite(o.epsilon))
        return fail(ctx, POLEE_ERR_BAD_ARG, "polee_tsne: an option is out of range");
    return POLEE_OK;
}

polee_status ensure_batch(polee_tsne *ts, int32_t B)
{
    polee_ctx *ctx = ts->ctx;
    const int64_t pw = tile_pairs(B) * ceil_div(ts->n, TS_CHUNK);
    if (pw > 0x7fffffffll) return fail(ctx, POLEE_ERR_UNSUPPORTED, "polee_tsne: %lld workgroups in the pairwise pass", (long long)pw);
    POLEE_TRY(ts->d_pw.alloc(ctx, (size_t)pw * TS_ROWS * TS_ROWS));
    POLEE_TRY(ts->d_delta.alloc(ctx, (size_t)B * B));
    POLEE_TRY(ts->d_R.alloc(ctx, (size_t)B * B));
    POLEE_TRY(ts->d_cs.alloc(ctx, (size_t)B));
    POLEE_TRY(ts->d_lossrow.alloc(ctx, (size_t)B));
    POLEE_TRY(ts->d_trow.alloc(ctx, (size_t)B));
    return POLEE_OK;
}

// batches i32 [niter][B]: every index in 0 .. S-1, none twice within a batch
polee_status upload_batches(polee_tsne *ts, const int32_t *batches, int32_t B, int32_t niter)
{
    polee_ctx *ctx = ts->ctx;
    if (!batches) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_tsne: null batch");
    if (B < 2 || B > ts->S) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_tsne: batch size %d; it must be 2 .. S = %d", B, ts->S);
    std::vector<int32_t> seen((size_t)ts->S, -1);
    for (int32_t it = 0; it < niter; ++it)
        for (int32_t b = 0; b < B; ++b) {
            const int32_t s = batches[(size_t)it * B + b];
            if (s < 0 || s >= ts->S)
                return fail(ctx, POLEE_ERR_BAD_ARG, "polee_tsne: batch %d holds the index %d; S = %d", it, s, ts->S);
            if (seen[(size_t)s] == it) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_tsne: batch %d holds the index %d twice", it, s);
            seen[(size_t)s] = it;
        }
    POLEE_TRY(ensure_batch(ts, B));
    return ts->d_idx.upload(ctx, batches, (size_t)niter * B);
}

polee_status need_sigmas(polee_tsne *ts)
{
    if (!ts->have_sigmas) return fail(ts->ctx, POLEE_ERR_BAD_ARG, "polee_tsne: the bandwidths are not set (polee_tsne_set_sigmas)");
    return POLEE_OK;
}

polee_status upload_points(polee_tsne *ts, const float *x)
{
    POLEE_TRY(check_points(ts->ctx, "polee_tsne", x, ts->S, ts->n));
    return ts->d_x.upload(ts->ctx, x, (size_t)ts->S * ts->n);
}

// ap must be the model's S x n, on its context
polee_status approx_fits(polee_tsne *ts, polee_approx *ap)
{
    int32_t S = 0;
    return check_approx(ts->ctx, "polee_tsne", ap, ts->n, ts->S, &S);
}

// z (and the row means) of one x; d_idx [B] or null
template <int KP>
polee_status project_t(polee_tsne *ts, const float *d_x, int is_log, const int32_t *d_idx, int32_t B, bool accumulate)
{
    polee_ctx *ctx = ts->ctx;
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL((tsne_project_kernel<KP>), dim3((unsigned)ceil_div(ts->nchunks, DM_BLOCK / 64)), dim3(DM_BLOCK), 0, st, ts->n, ts->S,
                       ts->C, ts->nchunks, d_x, is_log, (const float *)ts->d_W.p, ts->d_part.p, ts->d_rpart.p);
    hipLaunchKernelGGL((tsne_finish_kernel<KP>), dim3((unsigned)ts->S), dim3(DM_BLOCK), 0, st, ts->n, ts->S, ts->C, ts->nchunks,
                       ts->o.use_vlr, (const float *)ts->d_part.p, (const float *)ts->d_rpart.p, d_idx, B, ts->d_z.p,
                       accumulate ? ts->d_zacc.p : nullptr, ts->d_mhat.p, ts->d_resid.p, ts->d_pos.p);
    POLEE_KERNEL_CHECK(ctx);
    return POLEE_OK;
}

// delta [B][B] of the rows d_idx of one x, after project_t
polee_status pairwise(polee_tsne *ts, const float *d_x, int is_log, const int32_t *d_idx, int32_t B)
{
    polee_ctx *ctx = ts->ctx;
    hipStream_t st = ctx->stream;
    const int nch = (int)ceil_div(ts->n, TS_CHUNK);
    const int64_t ntp = tile_pairs(B);
    hipLaunchKernelGGL(tsne_pairwise_kernel, dim3((unsigned)(ntp * nch)), dim3(DM_BLOCK), 0, st, ts->n, B, nch, d_x, is_log, d_idx,
                       (const float *)ts->d_mhat.p, ts->d_pw.p);
    hipLaunchKernelGGL(tsne_delta_kernel, dim3((unsigned)(ntp * TS_ROWS)), dim3(DM_BLOCK), 0, st, ts->n, B, nch, ts->o.use_vlr,
                       (const float *)ts->d_pw.p, d_idx, (const double *)ts->d_resid.p, ts->d_delta.p);
    POLEE_KERNEL_CHECK(ctx);
    return POLEE_OK;
}

// one evaluation through the kernels.  mode 0: Adam step number t; mode 1: the gradient goes to d_gout
template <int KP>
polee_status step_t(polee_tsne *ts, const float *d_x, int is_log, const int32_t *d_idx, int32_t B, int mode, int64_t t, float *d_loss_out)
{
    polee_ctx *ctx = ts->ctx;
    hipStream_t st = ctx->stream;
    const polee_tsne_opts &o = ts->o;
    const int32_t S = ts->S, C = ts->C;
    POLEE_TRY(project_t<KP>(ts, d_x, is_log, d_idx, B, false));
    POLEE_TRY(pairwise(ts, d_x, is_log, d_idx, B));
    hipLaunchKernelGGL(tsne_sums_kernel, dim3((unsigned)(B + S)), dim3(DM_BLOCK), 0, st, S, B, C, (double)o.alpha,
                       (const double *)ts->d_delta.p, d_idx, (const float *)ts->d_sigma.p, (const double *)ts->d_z.p, ts->d_cs.p,
                       ts->d_rowk.p);
    hipLaunchKernelGGL(tsne_loss_kernel, dim3((unsigned)B), dim3(DM_BLOCK), 0, st, S, B, C, (double)o.alpha, (double)o.eps,
                       (const double *)ts->d_delta.p, d_idx, (const float *)ts->d_sigma.p, (const double *)ts->d_z.p,
                       (const double *)ts->d_cs.p, (const double *)ts->d_rowk.p, ts->d_R.p, ts->d_lossrow.p, ts->d_trow.p, ts->d_Z.p);
    hipLaunchKernelGGL((tsne_dz_kernel<KP>), dim3((unsigned)S), dim3(DM_BLOCK), 0, st, S, B, C, (double)o.alpha,
                       (const double *)ts->d_z.p, (const int32_t *)ts->d_pos.p, (const double *)ts->d_R.p,
                       (const double *)ts->d_lossrow.p, (const double *)ts->d_trow.p, (const double *)ts->d_Z.p, ts->d_dz.p, d_loss_out);
    const double lr_t = mode == 0 ? tf_adam_rate(o.learning_rate, o.beta1, o.beta2, t) : 0.0;
    hipLaunchKernelGGL((tsne_grad_update_kernel<KP>), dim3((unsigned)ceil_div(ts->n, DM_BLOCK)), dim3(DM_BLOCK), 0, st, ts->n, S, C, d_x,
                       is_log, (const float *)ts->d_dz.p, ts->d_W.p, ts->d_M.p, ts->d_V.p, (float)lr_t, o.beta1, o.beta2, o.epsilon, mode,
                       ts->d_gout.p);
    POLEE_KERNEL_CHECK(ctx);
    return POLEE_OK;
}

polee_status step(polee_tsne *ts, const float *d_x, int is_log, const int32_t *d_idx, int32_t B, int mode, int64_t t, float *d_loss_out)
{
    return dispatch_kp(ts->KP, [&](auto kp) { return step_t<decltype(kp)::value>(ts, d_x, is_log, d_idx, B, mode, t, d_loss_out); });
}

polee_status project(polee_tsne *ts, const float *d_x, int is_log, const int32_t *d_idx, int32_t B, bool accumulate)
{
    return dispatch_kp(ts->KP, [&](auto kp) { return project_t<decltype(kp)::value>(ts, d_x, is_log, d_idx, B, accumulate); });
}

polee_status distances_of(polee_tsne *ts, const float *d_x, int is_log, double *delta)
{
    polee_ctx *ctx = ts->ctx;
    const int32_t S = ts->S;
    std::vector<int32_t> all((size_t)S);
    for (int32_t s = 0; s < S; ++s) all[(size_t)s] = s;
    POLEE_TRY(ensure_batch(ts, S));
    POLEE_TRY(ts->d_idx.upload(ctx, all));
    POLEE_TRY(project(ts, d_x, is_log, ts->d_idx.p, S, false));
    POLEE_TRY(pairwise(ts, d_x, is_log, ts->d_idx.p, S));
    return ts->d_delta.download(ctx, delta, (size_t)S * S);
}

polee_status eval_of(polee_tsne *ts, const float *d_x, int is_log, int32_t B, float *loss, float *g_w)
{
    polee_ctx *ctx = ts->ctx;
    POLEE_TRY(ts->d_loss.alloc(ctx, 1));
    POLEE_TRY(step(ts, d_x, is_log, ts->d_idx.p, B, 1, 0, ts->d_loss.p));
    POLEE_TRY(ts->d_loss.download(ctx, loss, 1));
    if (!g_w) return POLEE_OK;
    std::vector<float> flat((size_t)ts->cn);
    POLEE_TRY(ts->d_gout.download(ctx, flat.data(), flat.size()));
    wT_to_abi(flat.data(), ts->n, ts->C, g_w);
    return POLEE_OK;
}

polee_status embed_finish(polee_tsne *ts, int32_t ndraws, float *z)
{
    polee_ctx *ctx = ts->ctx;
    const int64_t sc = (int64_t)ts->S * ts->C;
    POLEE_TRY(launch_acc_mean(ctx, sc, ts->d_zacc.p, ndraws, ts->d_zout.p));
    return ts->d_zout.download(ctx, z, (size_t)sc);
}

}  // namespace

extern "C" {

void polee_tsne_default_opts(polee_tsne_opts *o)
{
    if (!o) return;
    o->num_components = 2;     // --num-components (tsne.jl:23-27)
    o->use_vlr = 1;            // (tsne.jl:94)
    o->alpha = 1.0f;           // (polee_tsne.py:218)
    o->eps = 1e-6f;            // added to P and to Q (:309, :319, :327)
    o->learning_rate = 1e-6f;  // tf.train.AdamOptimizer(1e-6, beta1=0.99, beta2=0.999) (:344-345)
    o->beta1 = 0.99f;
    o->beta2 = 0.999f;
    o->epsilon = 1e-8f;        // (TF1's default)
}

polee_status polee_tsne_create(polee_ctx *ctx, int32_t n, int32_t S, const polee_tsne_opts *opts, polee_tsne **out)
{
    return ctx_entry(ctx, "polee_tsne_create", [&]() -> polee_status {
        if (!out || n < 2 || S < 2) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_tsne_create: bad argument");
        polee_tsne_opts o;
        polee_tsne_default_opts(&o);
        if (opts) o = *opts;
        const int32_t C = o.num_components;
        if (C < 1 || C > 16)
            return fail(ctx, POLEE_ERR_UNSUPPORTED, "polee_tsne_create: %d components; the kernels are built for 1..16", C);
        POLEE_TRY(check_opts(ctx, o));
        polee_tsne *ts = new polee_tsne();
        ts->ctx = ctx;
        ctx_retain(ctx);
        ts->n = n;
        ts->S = S;
        ts->C = C;
        ts->KP = kp_of(C);
        ts->nchunks = (int32_t)ceil_div(n, DM_WAVE_J);
        ts->cn = (int64_t)C * n;
        ts->o = o;
        polee_status st = POLEE_OK;
        auto A = [&](polee_status s) {
            if (st == POLEE_OK) st = s;
        };
        const size_t cn = (size_t)ts->cn, sc = (size_t)S * C;
        A(ts->d_W.alloc(ctx, cn));
        A(ts->d_M.alloc(ctx, cn));
        A(ts->d_V.alloc(ctx, cn));
        A(ts->d_gout.alloc(ctx, cn));
        A(ts->d_part.alloc(ctx, (size_t)ts->nchunks * sc));
        A(ts->d_rpart.alloc(ctx, (size_t)ts->nchunks * S));
        A(ts->d_mhat.alloc(ctx, (size_t)S));
        A(ts->d_sigma.alloc(ctx, (size_t)S));
        A(ts->d_dz.alloc(ctx, sc));
        A(ts->d_zout.alloc(ctx, sc));
        A(ts->d_loss.alloc(ctx, 1));
        A(ts->d_z.alloc(ctx, sc));
        A(ts->d_zacc.alloc(ctx, sc));
        A(ts->d_resid.alloc(ctx, (size_t)S));
        A(ts->d_rowk.alloc(ctx, (size_t)S));
        A(ts->d_Z.alloc(ctx, 1));
        A(ts->d_pos.alloc(ctx, (size_t)S));
        if (st == POLEE_OK) {
            hipError_t e = hipSuccess;
            for (float *p : {ts->d_W.p, ts->d_M.p, ts->d_V.p})
                if (e == hipSuccess) e = hipMemsetAsync(p, 0, cn * sizeof(float), ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) st = fail(ctx, POLEE_ERR_HIP, "polee_tsne_create: %s", hipGetErrorString(e));
        }
        if (st != POLEE_OK) {
            polee_tsne_destroy(ts);
            return st;
        }
        *out = ts;
        return POLEE_OK;
    });
}

void polee_tsne_destroy(polee_tsne *ts)
{
    if (!ts) return;
    polee_ctx *ctx = ts->ctx;
    if (ctx) (void)hipSetDevice(ctx->device);
    delete ts;
    ctx_release(ctx);
}

polee_status polee_tsne_get_params(polee_tsne *ts, float *w)
{
    return entry(ts, "polee_tsne_get_params", [&](polee_ctx *ctx) -> polee_status {
        if (!w) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_tsne_get_params: null argument");
        std::vector<float> flat((size_t)ts->cn);
        POLEE_TRY(ts->d_W.download(ctx, flat.data(), flat.size()));
        wT_to_abi(flat.data(), ts->n, ts->C, w);
        return POLEE_OK;
    });
}

polee_status polee_tsne_set_params(polee_tsne *ts, const float *w)
{
    return entry(ts, "polee_tsne_set_params", [&](polee_ctx *ctx) -> polee_status {
        if (!w) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_tsne_set_params: null argument");
        std::vector<float> flat((size_t)ts->cn);
        abi_to_wT(w, ts->n, ts->C, flat.data());
        return ts->d_W.upload(ctx, flat);
    });
}

polee_status polee_tsne_reset(polee_tsne *ts)
{
    return entry(ts, "polee_tsne_reset", [&](polee_ctx *ctx) -> polee_status {
        const size_t bytes = (size_t)ts->cn * sizeof(float);
        POLEE_HIP_TRY(ctx, hipMemsetAsync(ts->d_M.p, 0, bytes, ctx->stream));
        POLEE_HIP_TRY(ctx, hipMemsetAsync(ts->d_V.p, 0, bytes, ctx->stream));
        POLEE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        ts->t = 0;
        return POLEE_OK;
    });
}

polee_status polee_tsne_set_sigmas(polee_tsne *ts, const float *sigmas)
{
    return entry(ts, "polee_tsne_set_sigmas", [&](polee_ctx *ctx) -> polee_status {
        if (!sigmas) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_tsne_set_sigmas: null argument");
        for (int32_t s = 0; s < ts->S; ++s)
            if (!(sigmas[s] > 0.0f) || !std::isfinite(sigmas[s]))
                return fail(ctx, POLEE_ERR_BAD_ARG, "polee_tsne_set_sigmas: sigma[%d] = %g is not positive and finite", s,
                            (double)sigmas[s]);
        POLEE_TRY(ts->d_sigma.upload(ctx, sigmas, (size_t)ts->S));
        ts->have_sigmas = true;
        return POLEE_OK;
    });
}

polee_status polee_tsne_distances(polee_tsne *ts, polee_approx *ap, const float *z0, uint64_t seed, double *delta)
{
    return entry(ts, "polee_tsne_distances", [&](polee_ctx *ctx) -> polee_status {
        POLEE_TRY(approx_fits(ts, ap));
        if (!delta) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_tsne_distances: null argument");
        DrawFeed feed(ap, ts->d_z0, ts->S, ts->n, seed);
        const float *d_x = nullptr;
        POLEE_TRY(feed.upload(z0, 1));
        POLEE_TRY(feed.draw(0, 0, &d_x));
        return distances_of(ts, d_x, 0, delta);
    });
}

polee_status polee_tsne_distances_points(polee_tsne *ts, const float *x, double *delta)
{
    return entry(ts, "polee_tsne_distances_points", [&](polee_ctx *ctx) -> polee_status {
        if (!delta) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_tsne_distances_points: null argument");
        POLEE_TRY(upload_points(ts, x));
        return distances_of(ts, ts->d_x.p, 1, delta);
    });
}

polee_status polee_tsne_eval(polee_tsne *ts, polee_approx *ap, const int32_t *batch, int32_t B, const float *z0, uint64_t seed,
                             float *loss, float *g_w)
{
    return entry(ts, "polee_tsne_eval", [&](polee_ctx *ctx) -> polee_status {
        POLEE_TRY(approx_fits(ts, ap));
        if (!loss) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_tsne_eval: null argument");
        POLEE_TRY(need_sigmas(ts));
        POLEE_TRY(upload_batches(ts, batch, B, 1));
        DrawFeed feed(ap, ts->d_z0, ts->S, ts->n, seed);
        const float *d_x = nullptr;
        POLEE_TRY(feed.upload(z0, 1));
        POLEE_TRY(feed.draw(0, 0, &d_x));
        return eval_of(ts, d_x, 0, B, loss, g_w);
    });
}

polee_status polee_tsne_eval_points(polee_tsne *ts, const float *x, const int32_t *batch, int32_t B, float *loss, float *g_w)
{
    return entry(ts, "polee_tsne_eval_points", [&](polee_ctx *ctx) -> polee_status {
        if (!loss) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_tsne_eval_points: null argument");
        POLEE_TRY(need_sigmas(ts));
        POLEE_TRY(upload_batches(ts, batch, B, 1));
        POLEE_TRY(upload_points(ts, x));
        return eval_of(ts, ts->d_x.p, 1, B, loss, g_w);
    });
}

// (a step keeps no sums from one step to the next: a call that fails partway has the updates of the steps it completed, and the
// clock advances by those)
polee_status polee_tsne_fit(polee_tsne *ts, polee_approx *ap, const int32_t *batches, int32_t B, int32_t niter, uint64_t seed,
                            const float *z0, float *loss_trace)
{
    return entry(ts, "polee_tsne_fit", [&](polee_ctx *ctx) -> polee_status {
        POLEE_TRY(approx_fits(ts, ap));
        if (niter < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_tsne_fit: niter < 1");
        POLEE_TRY(need_sigmas(ts));
        POLEE_TRY(upload_batches(ts, batches, B, niter));
        POLEE_TRY(ts->d_loss.alloc(ctx, (size_t)niter));
        DrawFeed feed(ap, ts->d_z0, ts->S, ts->n, seed);
        const float *d_x = nullptr;
        POLEE_TRY(feed.upload(z0, (size_t)niter));
        for (int32_t it = 0; it < niter; ++it) {
            const int64_t t = ts->t + it + 1;
            polee_status st = feed.draw((uint64_t)(t - 1), (size_t)it, &d_x);
            if (st == POLEE_OK) st = step(ts, d_x, 0, ts->d_idx.p + (size_t)it * B, B, 0, t, ts->d_loss.p + it);
            if (st != POLEE_OK) {
                ts->t += it;
                return st;
            }
        }
        return fit_finish(ctx, &ts->t, ts->d_loss, niter, loss_trace);
    });
}

polee_status polee_tsne_fit_points(polee_tsne *ts, const float *x, const int32_t *batches, int32_t B, int32_t niter, float *loss_trace)
{
    return entry(ts, "polee_tsne_fit_points", [&](polee_ctx *ctx) -> polee_status {
        if (niter < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_tsne_fit_points: niter < 1");
        POLEE_TRY(need_sigmas(ts));
        POLEE_TRY(upload_batches(ts, batches, B, niter));
        POLEE_TRY(upload_points(ts, x));
        POLEE_TRY(ts->d_loss.alloc(ctx, (size_t)niter));
        for (int32_t it = 0; it < niter; ++it) {
            const polee_status st = step(ts, ts->d_x.p, 1, ts->d_idx.p + (size_t)it * B, B, 0, ts->t + it + 1, ts->d_loss.p + it);
            if (st != POLEE_OK) {
                ts->t += it;
                return st;
            }
        }
        return fit_finish(ctx, &ts->t, ts->d_loss, niter, loss_trace);
    });
}

polee_status polee_tsne_embed(polee_tsne *ts, polee_approx *ap, int32_t ndraws, uint64_t seed, const float *z0, float *z)
{
    return entry(ts, "polee_tsne_embed", [&](polee_ctx *ctx) -> polee_status {
        POLEE_TRY(approx_fits(ts, ap));
        if (!z || ndraws < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_tsne_embed: bad argument");
        DrawFeed feed(ap, ts->d_z0, ts->S, ts->n, seed);
        const float *d_x = nullptr;
        POLEE_TRY(feed.upload(z0, (size_t)ndraws));
        POLEE_HIP_TRY(ctx, hipMemsetAsync(ts->d_zacc.p, 0, (size_t)ts->S * ts->C * sizeof(double), ctx->stream));
        for (int32_t i = 0; i < ndraws; ++i) {
            POLEE_TRY(feed.draw((uint64_t)i, (size_t)i, &d_x));
            POLEE_TRY(project(ts, d_x, 0, nullptr, 0, true));
        }
        return embed_finish(ts, ndraws, z);
    });
}

polee_status polee_tsne_embed_points(polee_tsne *ts, const float *x, float *z)
{
    return entry(ts, "polee_tsne_embed_points", [&](polee_ctx *ctx) -> polee_status {
        if (!z) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_tsne_embed_points: null argument");
        POLEE_TRY(upload_points(ts, x));
        POLEE_HIP_TRY(ctx, hipMemsetAsync(ts->d_zacc.p, 0, (size_t)ts->S * ts->C * sizeof(double), ctx->stream));
        POLEE_TRY(project(ts, ts->d_x.p, 1, nullptr, 0, true));
        return embed_finish(ts, 1, z);
    });
}

}  // extern "C"
