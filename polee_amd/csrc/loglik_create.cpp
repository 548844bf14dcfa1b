// Creation of the likelihood handle: X by columns or by rows, from the host or from device memory, into the PSELL layout
// (built on the device, psell_device.hip, or by the host builder, psell_build.cpp), uploaded, with the streaming kernel's
// schedule (loglik.hip) prepared.  Host code only: built like the other .cpp files, without loglik.hip's tuning flags.
#include "loglik_internal.hpp"
#include "psell_device.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>

using namespace polee;

static double wall_now()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static polee_status loglik_finish_create(polee_ctx *ctx, polee_loglik *ll, polee_loglik **out)
{
    PsellHost &h = ll->host;
    polee_status s;
    static const bool timing = getenv("POLEE_BUILD_TIMING") != nullptr;
    const double t_begin = wall_now();
    if (!ll->device_built) h.data.resize(h.data.size() + 2048, 0);  // slack: the LDS-DMA stream reads whole 1 KiB pieces
    // (device_built: the slice stream and the multiplicities were laid out on the device, psell_device.hip, and are in place)
    if ((!ll->device_built && (s = ll->d_data.upload(ctx, h.data.data(), h.data.size()))) || (s = ll->d_slice_off.upload(ctx, h.slice_off)) ||
        (s = ll->d_tile_slice.upload(ctx, h.tile_slice)) || (s = ll->d_tile_dict.upload(ctx, h.tile_dict)) ||
        (s = ll->d_dict.upload(ctx, h.dict)) ||
        (ll->has_ks && !ll->device_built && (s = ll->d_slice_ks.upload(ctx, h.slice_ks))) ||
        (!h.csr_rows.empty() && ((s = ll->d_csr_rowptr.upload(ctx, h.csr_rowptr)) || (s = ll->d_csr_col.upload(ctx, h.csr_col)) ||
                                 (s = ll->d_csr_val.upload(ctx, h.csr_val)) || (ll->has_ks && (s = ll->d_csr_ks.upload(ctx, h.csr_ks)))))) {
        loglik_release(ll);
        return s;
    }
    ll->csr_rows = (int64_t)h.csr_rows.size();
    ll->csr_nnz = (int64_t)h.csr_col.size();
    if (!h.single_cnt.empty()) {
        if ((s = ll->d_single_cnt.upload(ctx, h.single_cnt)) ||
            (s = ll->d_single_part.alloc(ctx, (size_t)ceil_div(ll->n, SINGLE_THREADS) * PSELL_MAX_K))) {
            loglik_release(ll);
            return s;
        }
        ll->has_singles = true;
        std::vector<float>().swap(h.single_cnt);
    }
    if (timing) fprintf(stderr, "[loglik create] %-28s %.3f s\n", "upload", wall_now() - t_begin);
    // what the streaming kernel's schedule needs, before the bulk vectors go: the relative cost of every tile
    // (bytes it streams; the latency-bound streams weigh more per byte), the x windows, the usual grid's schedule
    ll->dict_len = (int64_t)h.dict.size();
    loglik_prepare_tiles(ll);
    {   // deterministic mode: the dictionary entries of every transcript, ascending (= tile order), padding left out
        std::vector<uint32_t> ptr((size_t)ll->n + 1, 0), slots;
        for (int64_t t = 0; t < h.num_tiles; ++t)  // (stream B's tiles too: their sums go through gwin in the deterministic mode)
            for (uint32_t l = 0; l < h.tile_cols[t]; ++l) ++ptr[(size_t)h.dict[h.tile_dict[t] + l] + 1];
        for (int64_t j = 0; j < ll->n; ++j) ptr[(size_t)j + 1] += ptr[(size_t)j];
        slots.resize(ptr[(size_t)ll->n]);
        std::vector<uint32_t> cur(ptr.begin(), ptr.end() - 1);
        for (int64_t t = 0; t < h.num_tiles; ++t)
            for (uint32_t l = 0; l < h.tile_cols[t]; ++l) {
                const uint32_t e = h.tile_dict[t] + l;
                slots[cur[h.dict[e]]++] = e;
            }
        std::vector<uint32_t> heavy;
        for (int64_t j = 0; j < ll->n; ++j)
            if (ptr[(size_t)j + 1] - ptr[(size_t)j] > GWIN_HEAVY) heavy.push_back((uint32_t)j);
        if ((s = ll->d_tslot_ptr.upload(ctx, ptr)) || (s = ll->d_tslot.upload(ctx, slots)) || (s = ll->d_theavy.upload(ctx, heavy))) {
            loglik_release(ll);
            return s;
        }
    }
    if ((s = ll->d_xwin.alloc(ctx, (size_t)ll->dict_len * PSELL_MAX_K + 512)) ||
        // (the dictionaries' padding entries are never referenced by a slice; they are read into LDS with their tile's
        // window, and the VI loop's forward kernel -- which fills the windows through the slot lists -- does not write them)
        (hipMemsetAsync(ll->d_xwin.p, 0, ((size_t)ll->dict_len * PSELL_MAX_K + 512) * sizeof(float), ctx->stream) != hipSuccess &&
         (s = fail(ctx, POLEE_ERR_HIP, "hipMemset failed")) != POLEE_OK) ||
        (s = loglik_ensure_schedule(ll, (int)std::min<int64_t>((int64_t)4 * ctx->num_cus, std::max<int64_t>(h.num_tiles, 1))))) {
        loglik_release(ll);
        return s;
    }
    if (timing) fprintf(stderr, "[loglik create] %-28s %.3f s\n", "upload + schedule + lists", wall_now() - t_begin);
    // keep only metadata on the host
    decltype(h.data)().swap(h.data);
    std::vector<uint32_t>().swap(h.slice_off);
    std::vector<uint32_t>().swap(h.dict);
    std::vector<float>().swap(h.slice_ks);
    std::vector<uint8_t>().swap(h.slice_flags);
    std::vector<uint8_t>().swap(h.slice_w);
    std::vector<uint32_t>().swap(h.row_order);
    std::vector<uint32_t>().swap(h.csr_rowptr);
    std::vector<uint32_t>().swap(h.csr_col);
    std::vector<uint32_t>().swap(h.csr_rows);
    std::vector<float>().swap(h.csr_val);
    std::vector<float>().swap(h.csr_ks);
    *out = ll;
    return POLEE_OK;
}

namespace polee {
// CSC (1-based, as in the HDF5) -> CSR (0-based).  Columns stay ascending within a row.
std::string csc_to_csr(int64_t m, int64_t n, const void *colptr, int colptr_bytes, const uint32_t *rowval,
                       const float *nzval, BVec<uint64_t> &rowptr, RawVec<uint32_t> &col, RawVec<float> &val)
{
    auto cp = [&](int64_t j) -> uint64_t {
        return colptr_bytes == 4 ? (uint64_t) reinterpret_cast<const uint32_t *>(colptr)[j]
                                 : reinterpret_cast<const uint64_t *>(colptr)[j];
    };
    if (colptr_bytes != 4 && colptr_bytes != 8) return "colptr_bytes must be 4 or 8";
    if (cp(0) != 1) return "colptr[0] must be 1 (1-based)";
    const double t_enter = wall_now();
    const uint64_t nnz = cp(n) - 1;
    for (int64_t j = 0; j < n; ++j)
        if (cp(j + 1) < cp(j)) return "colptr is not monotone";
    rowptr.assign(m + 1, 0);
    // Transposition in two partitioned passes on the host threads, without atomics and without a sort:
    //   the columns are cut into chunks of equal nnz, the rows into buckets of 2^sh consecutive rows (a bucket's cursors
    //   stay in a core's L2);
    //   pass 1: every chunk counts its entries per bucket; a prefix over (bucket, chunk) gives every (chunk, bucket) pair
    //           its own contiguous piece of a staging array, bucket-major, chunks in column order inside a bucket;
    //   pass 2: every chunk writes (row, column, value) records into its pieces -- a few hundred sequential write
    //           streams per thread instead of 240 M random ones;
    //   pass 3: every bucket counts its rows, prefixes (that IS its part of rowptr) and places its records: they arrive
    //           in ascending column order, so every row comes out sorted by transcript, as a sequential transposition
    //           would leave it.
    col.clear();
    val.clear();
    if (nnz == 0) return "";
    if (m < 1) return "rowval out of range";
    static const bool timing = getenv("POLEE_BUILD_TIMING") != nullptr;
    double t_prev = t_enter;
    auto lap = [&](const char *what) {
        if (timing) fprintf(stderr, "[CSC -> rows] %-30s %.3f s\n", what, wall_now() - t_prev);
        t_prev = wall_now();
    };
    int sh = 0;
    while (((uint64_t)m >> sh) > 512) ++sh;  // <= 512 buckets (+1)
    if (sh < 12) sh = 12;
    const size_t B = (size_t)(((uint64_t)m - 1) >> sh) + 1;
    const size_t NC = std::max<size_t>(1, std::min<size_t>(4 * host_threads(), (size_t)(nnz >> 16) + 1));
    std::vector<int64_t> cstart(NC + 1, n);  // chunk c = columns [cstart[c], cstart[c+1])
    for (size_t c = 0; c <= NC; ++c) {
        const uint64_t target = 1 + nnz * c / NC;  // first column whose start is >= target
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) / 2;
            if (cp(mid) < target) lo = mid + 1; else hi = mid;
        }
        cstart[c] = c == NC ? n : lo;
    }
    cstart[0] = 0;
    std::vector<uint64_t> cnt(NC * B, 0);
    std::atomic<int> err{0};
    parallel_chunks(NC, 1, [&](size_t clo, size_t chi, unsigned) {
        for (size_t c = clo; c < chi; ++c) {
            uint64_t *cc = cnt.data() + c * B;
            for (uint64_t k = cp(cstart[c]) - 1; k < cp(cstart[c + 1]) - 1; ++k) {
                const uint32_t r = rowval[k];
                if (r < 1 || (int64_t)r > m) {
                    err = 1;
                    continue;
                }
                ++cc[(r - 1) >> sh];
            }
        }
    });
    if (err) return "rowval out of range";
    lap("checks + count per (chunk, bucket)");
    std::vector<uint64_t> bstart(B + 1, 0);
    {
        uint64_t run = 0;
        for (size_t b = 0; b < B; ++b) {
            bstart[b] = run;
            for (size_t c = 0; c < NC; ++c) {
                const uint64_t t = cnt[c * B + b];
                cnt[c * B + b] = run;  // becomes the write cursor of (chunk, bucket)
                run += t;
            }
        }
        bstart[B] = run;
    }
    struct Rec {
        uint32_t row, col;
        float val;
    };
    std::vector<Rec, default_init_allocator<Rec>> stage((size_t)nnz);
    lap("allocate staging");
    parallel_chunks(NC, 1, [&](size_t clo, size_t chi, unsigned) {
        for (size_t c = clo; c < chi; ++c) {
            uint64_t *cur = cnt.data() + c * B;
            for (int64_t j = cstart[c]; j < cstart[c + 1]; ++j)
                for (uint64_t k = cp(j) - 1; k < cp(j + 1) - 1; ++k) {
                    const uint32_t r = rowval[k] - 1;
                    stage[cur[r >> sh]++] = Rec{r, (uint32_t)j, nzval[k]};
                }
        }
    });
    lap("scatter into buckets");
    col.resize(nnz);
    val.resize(nnz);
    lap("allocate rows");
    parallel_chunks(B, 1, [&](size_t blo, size_t bhi, unsigned) {
        std::vector<uint32_t> local;
        for (size_t b = blo; b < bhi; ++b) {
            const uint64_t r0 = (uint64_t)b << sh, r1 = std::min<uint64_t>((uint64_t)m, r0 + ((uint64_t)1 << sh));
            local.assign((size_t)(r1 - r0) + 1, 0);
            for (uint64_t p = bstart[b]; p < bstart[b + 1]; ++p) ++local[stage[p].row - r0 + 1];
            for (size_t i = 1; i < local.size(); ++i) local[i] += local[i - 1];
            for (uint64_t i = 0; i < r1 - r0; ++i) rowptr[r0 + i + 1] = bstart[b] + local[i + 1];
            for (uint64_t p = bstart[b]; p < bstart[b + 1]; ++p) {
                const Rec &e = stage[p];
                const uint64_t q = bstart[b] + local[e.row - r0]++;
                col[q] = e.col;
                val[q] = e.val;
            }
        }
    });
    rowptr[0] = 0;
    lap("place within buckets");
    return "";
}
}  // namespace polee

extern "C" {

// A fresh handle on ctx (one reference, the context retained)
static polee_status new_handle(polee_ctx *ctx, int64_t m, int64_t n, int64_t nnz, bool has_ks, polee_loglik *&ll)
{
    ll = new (std::nothrow) polee_loglik();
    if (!ll) return fail(ctx, POLEE_ERR_OOM, "out of host memory");
    ll->ctx = ctx;
    ctx_retain(ctx);
    ll->m = m;
    ll->n = n;
    ll->nnz = nnz;
    ll->has_ks = has_ks;
    return POLEE_OK;
}

// The host builder's layout of X by rows (0-based) into the handle, then the uploads; a failure releases the handle
static polee_status build_on_host(polee_ctx *ctx, polee_loglik *ll, const uint64_t *rowptr, const uint32_t *col, const float *val,
                                  const int64_t *ks, polee_loglik **out)
{
    const std::string err = build_psell(ll->m, ll->n, rowptr, col, val, ks, ll->host);
    if (!err.empty()) {
        loglik_release(ll);
        return fail(ctx, err.find("more than") != std::string::npos ? POLEE_ERR_UNSUPPORTED : POLEE_ERR_BAD_ARG,
                    "likelihood matrix: %s", err.c_str());
    }
    return loglik_finish_create(ctx, ll, out);
}

// The layout built on the device from X by rows in device memory (psell_device.hip).  done = false (and POLEE_OK): the matrix
// is the host builder's case -- a real share of fragments without any structure.
static polee_status loglik_create_on_device(polee_ctx *ctx, const PsellDevIn &X, bool has_ks, polee_loglik **out, bool &done)
{
    done = false;
    polee_loglik *ll = nullptr;
    POLEE_TRY(new_handle(ctx, X.m, X.n, 0, has_ks, ll));  // (nnz: the builder counts them)
    PsellDevOut D;
    bool needs_host = false;
    polee_status st = psell_device_build(ctx, X, ll->host, D, false, needs_host);
    if (st != POLEE_OK || needs_host) {
        loglik_release(ll);
        return st;
    }
    ll->nnz = ll->host.nnz;
    ll->device_built = true;
    ll->d_data.take(D.data);
    if (has_ks) ll->d_slice_ks.take(D.slice_ks);
    done = true;
    return loglik_finish_create(ctx, ll, out);
}

static polee_status polee_loglik_create_from_xt_impl(polee_ctx *ctx, int64_t m, int64_t n, const uint64_t *tcolptr,
                                         const uint32_t *trowval, const float *tnzval, const int64_t *ks,
                                         polee_loglik **out)
{
    POLEE_TRY(use_device(ctx));
    if (!tcolptr || !out || m < 0 || n < 1 || (tcolptr[m] > 1 && (!trowval || !tnzval)))
        return fail(ctx, POLEE_ERR_BAD_ARG, "polee_loglik_create_from_xt: bad argument");
    if (tcolptr[0] != 1) return fail(ctx, POLEE_ERR_BAD_ARG, "tcolptr[0] must be 1 (1-based)");
    const uint64_t nnz = tcolptr[m] - 1;
    const double t_begin = wall_now();
    if (psell_device_enabled() && nnz < (1ull << 32) - 1 && m < ((int64_t)1 << 32) - 1) {
        polee_status st = POLEE_OK;
        bool done = false;
        {
            PsellDevCSR C;
            if ((st = psell_device_rows_from_xt(ctx, m, n, tcolptr, trowval, tnzval, ks, false, C)) != POLEE_OK) return st;
            st = loglik_create_on_device(ctx, C.view(), ks != nullptr, out, done);
        }
        if (st != POLEE_OK || done) return st;
    }
    // (0-based copies; vectors that do not zero-fill a gigabyte first, filled on several threads)
    std::vector<uint64_t, default_init_allocator<uint64_t>> rowptr(m + 1);
    parallel_chunks((size_t)m + 1, (size_t)1 << 20, [&](size_t lo, size_t hi, unsigned) {
        for (size_t i = lo; i < hi; ++i) rowptr[i] = tcolptr[i] - 1;
    });
    std::vector<uint32_t, default_init_allocator<uint32_t>> col(nnz);
    {
        std::atomic<int> bad{0};
        parallel_chunks((size_t)nnz, (size_t)1 << 20, [&](size_t lo, size_t hi, unsigned) {
            for (size_t k = lo; k < hi; ++k) {
                if (trowval[k] < 1) bad = 1;
                col[k] = trowval[k] - 1;
            }
        });
        if (bad) return fail(ctx, POLEE_ERR_BAD_ARG, "trowval must be 1-based");
    }
    polee_loglik *ll = nullptr;
    POLEE_TRY(new_handle(ctx, m, n, (int64_t)nnz, ks != nullptr, ll));
    if (getenv("POLEE_BUILD_TIMING")) fprintf(stderr, "[loglik create] %-28s %.3f s\n", "0-based copies of the input", wall_now() - t_begin);
    return build_on_host(ctx, ll, rowptr.data(), col.data(), tnzval, ks, out);
}

int polee_loglik_built_on_device(const polee_loglik *ll) { return ll && ll->device_built ? 1 : 0; }

static polee_status polee_loglik_create_from_xbuild_impl(polee_ctx *ctx, const polee_xbuild *xb, const int64_t *ks, polee_loglik **out)
{
    POLEE_TRY(use_device(ctx));
    if (!xb || !out) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_loglik_create_from_xbuild: null argument");
    polee_ctx *xctx = nullptr;
    int64_t m = 0, n = 0;
    const uint64_t *tcolptr = nullptr;
    const uint32_t *trowval = nullptr;
    const float *tnzval = nullptr;
    POLEE_TRY(xbuild_device_view(xb, &xctx, &m, &n, &tcolptr, &trowval, &tnzval));
    if (xctx->device != ctx->device) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_loglik_create_from_xbuild: the xbuild result lives on another device");
    POLEE_HIP_TRY(ctx, hipStreamSynchronize(xctx->stream));
    bool done = false;
    polee_status st = POLEE_OK;
    uint64_t nnz_dev = 0;  // (the device builder numbers non-zeros in 32 bits, as the from_xt path checks: ADVICE r4)
    if (m > 0) {
        POLEE_HIP_TRY(ctx, hipMemcpy(&nnz_dev, tcolptr + m, sizeof nnz_dev, hipMemcpyDeviceToHost));
        nnz_dev -= 1;
    }
    if (psell_device_enabled() && nnz_dev < (1ull << 32) - 1 && m < ((int64_t)1 << 32) - 1) {
        PsellDevCSR C;
        DevBuf<int64_t> d_ks;
        if (ks) POLEE_TRY(d_ks.upload(ctx, ks, (size_t)m));
        if ((st = psell_device_rows_from_xt(ctx, m, n, tcolptr, trowval, tnzval, ks ? d_ks.p : nullptr, true, C)) != POLEE_OK) return st;
        st = loglik_create_on_device(ctx, C.view(), ks != nullptr, out, done);
        if (st != POLEE_OK || done) return st;
    }
    // the host builder's case: through the host arrays
    std::vector<uint64_t> h_ptr((size_t)m + 1);
    POLEE_HIP_TRY(ctx, hipMemcpy(h_ptr.data(), tcolptr, ((size_t)m + 1) * 8, hipMemcpyDeviceToHost));
    const size_t nnz = (size_t)(h_ptr[(size_t)m] - 1);
    std::vector<uint32_t> h_col(nnz);
    std::vector<float> h_val(nnz);
    if (nnz) {
        POLEE_HIP_TRY(ctx, hipMemcpy(h_col.data(), trowval, nnz * 4, hipMemcpyDeviceToHost));
        POLEE_HIP_TRY(ctx, hipMemcpy(h_val.data(), tnzval, nnz * 4, hipMemcpyDeviceToHost));
    }
    return polee_loglik_create_from_xt(ctx, m, n, h_ptr.data(), h_col.data(), h_val.data(), ks, out);
}

polee_status polee_loglik_create_from_xbuild(polee_ctx *ctx, const polee_xbuild *xb, const int64_t *ks, polee_loglik **out)
{
    return ctx_entry(ctx, "polee_loglik_create_from_xbuild", [&]() -> polee_status {
        return polee_loglik_create_from_xbuild_impl(ctx, xb, ks, out);
    });
}

polee_status polee_loglik_create_from_xt(polee_ctx *ctx, int64_t m, int64_t n, const uint64_t *tcolptr,
                                         const uint32_t *trowval, const float *tnzval, const int64_t *ks,
                                         polee_loglik **out)
{
    return ctx_entry(ctx, "polee_loglik_create_from_xt", [&]() -> polee_status {
        return polee_loglik_create_from_xt_impl(ctx, m, n, tcolptr, trowval, tnzval, ks, out);
    });
}

static polee_status polee_loglik_create_impl(polee_ctx *ctx, int64_t m, int64_t n, const void *colptr, int colptr_bytes,
                                 const uint32_t *rowval, const float *nzval, const int64_t *ks, polee_loglik **out)
{
    POLEE_TRY(use_device(ctx));
    if (!colptr || !out || m < 0 || n < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_loglik_create: bad argument");
    BVec<uint64_t> rowptr;
    RawVec<uint32_t> col;  // (resize leaves them uninitialised: 1.9 GB of zeros would be written by one thread)
    RawVec<float> val;
    static const bool timing = getenv("POLEE_BUILD_TIMING") != nullptr;
    const double t_begin = wall_now();
    if (psell_device_enabled()) {
        polee_status st = POLEE_OK;
        bool done = false;
        {
            PsellDevCSR C;
            bool needs_host = false;
            if ((st = psell_device_rows_from_csc(ctx, m, n, colptr, colptr_bytes, rowval, nzval, ks, C, needs_host)) != POLEE_OK) return st;
            if (timing) fprintf(stderr, "[loglik create] %-28s %.3f s\n", "X onto the device, by rows", wall_now() - t_begin);
            if (!needs_host) st = loglik_create_on_device(ctx, C.view(), ks != nullptr, out, done);
        }
        if (timing && done) fprintf(stderr, "[loglik create] %-28s %.3f s\n", "total (device build)", wall_now() - t_begin);
        if (st != POLEE_OK || done) return st;
    }
    std::string err = csc_to_csr(m, n, colptr, colptr_bytes, rowval, nzval, rowptr, col, val);
    if (timing) fprintf(stderr, "[loglik create] %-28s %.3f s\n", "CSC -> rows", wall_now() - t_begin);
    if (!err.empty()) return fail(ctx, POLEE_ERR_BAD_ARG, "likelihood matrix: %s", err.c_str());
    polee_loglik *ll = nullptr;
    POLEE_TRY(new_handle(ctx, m, n, (int64_t)col.size(), ks != nullptr, ll));
    const polee_status st = build_on_host(ctx, ll, rowptr.data(), col.data(), val.data(), ks, out);
    if (timing) fprintf(stderr, "[loglik create] %-28s %.3f s\n", "total", wall_now() - t_begin);
    return st;
}

polee_status polee_loglik_create(polee_ctx *ctx, int64_t m, int64_t n, const void *colptr, int colptr_bytes,
                                 const uint32_t *rowval, const float *nzval, const int64_t *ks, polee_loglik **out)
{
    return ctx_entry(ctx, "polee_loglik_create", [&]() -> polee_status {
        return polee_loglik_create_impl(ctx, m, n, colptr, colptr_bytes, rowval, nzval, ks, out);
    });
}

// ---- X on the device, once, for the tree and the layout ------------------------------------------------------
polee_status polee_devx_upload(polee_ctx *ctx, int64_t m, int64_t n, const void *colptr, int colptr_bytes, const uint32_t *rowval,
                               const float *nzval, polee_devx **out)
{
    return ctx_entry(ctx, "polee_devx_upload", [&]() -> polee_status {
        if (!colptr || !out || m < 0 || n < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_devx_upload: bad argument");
        std::vector<uint64_t> cp;
        uint64_t nnz = 0;
        POLEE_TRY(psell_check_colptr(ctx, n, colptr, colptr_bytes, cp, nnz));
        if (nnz > 0 && !rowval) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_devx_upload: bad argument");
        if (nnz >= (1ull << 32) - 1 || m >= ((int64_t)1 << 32) - 1)
            return fail(ctx, POLEE_ERR_UNSUPPORTED, "polee_devx_upload: the device builders number rows and non-zeros in 32 bits (use polee_loglik_create / polee_hclust_parallel)");
        polee_devx *dx = new (std::nothrow) polee_devx();
        if (!dx) return fail(ctx, POLEE_ERR_OOM, "out of host memory");
        dx->ctx = ctx;
        dx->m = m;
        dx->n = n;
        dx->nnz = nnz;
        polee_status st = dx->cp.upload(ctx, cp.data(), cp.size());
        if (st == POLEE_OK && nnz) st = dx->rowval.upload(ctx, rowval, (size_t)nnz);
        if (st == POLEE_OK && nnz && nzval) st = dx->nzval.upload(ctx, nzval, (size_t)nnz);
        if (st != POLEE_OK) {
            delete dx;
            return st;
        }
        ctx_retain(ctx);
        *out = dx;
        return POLEE_OK;
    });
}

polee_status polee_devx_upload_values(polee_devx *dx, const float *nzval)
{
    return entry(dx, "polee_devx_upload_values", [&](polee_ctx *ctx) -> polee_status {
        if (dx->nnz && !nzval) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_devx_upload_values: null argument");
        if (dx->nnz) POLEE_TRY(dx->nzval.upload(ctx, nzval, (size_t)dx->nnz));
        return POLEE_OK;
    });
}

void polee_devx_destroy(polee_devx *dx)
{
    if (!dx) return;
    polee_ctx *ctx = dx->ctx;
    (void)hipSetDevice(ctx->device);
    dx->cp.release();
    dx->rowval.release();
    dx->nzval.release();
    delete dx;
    ctx_release(ctx);
}

polee_status polee_loglik_create_from_devx(polee_ctx *ctx, polee_devx *dx, const float *nzval, const int64_t *ks, polee_loglik **out)
{
    return ctx_entry(ctx, "polee_loglik_create_from_devx", [&]() -> polee_status {
        if (!dx || !out) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_loglik_create_from_devx: null argument");
        if (dx->ctx->device != ctx->device) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_loglik_create_from_devx: X lives on another device");
        if (dx->nnz && !dx->nzval.p && !nzval)
            return fail(ctx, POLEE_ERR_BAD_ARG, "polee_loglik_create_from_devx: the values have not been uploaded (polee_devx_upload_values, or pass them here)");
        const float *late = dx->nnz && !dx->nzval.p ? nzval : nullptr;  // (go up beside the first kernels, into the handle)
        // (device builder switched off -- POLEE_DEVICE_BUILD=0 or a host-builder knob: straight to the host layout builder below,
        // as polee_loglik_create would; the handle's copy of X still saves the tree builder its upload)
        if (psell_device_enabled()) {
            bool done = false;
            polee_status st = POLEE_OK;
            {
                PsellDevCSR C;
                if ((st = psell_device_rows_from_dev_csc(ctx, dx->m, dx->n, dx->cp.p, dx->nnz, dx->rowval.p, dx->nzval.p, ks, C, nullptr, late, &dx->nzval)) != POLEE_OK) return st;
                st = loglik_create_on_device(ctx, C.view(), ks != nullptr, out, done);
            }
            if (st != POLEE_OK || done) return st;
        }
        // the host builder's case (a real share of rows without any structure): through host arrays, as polee_loglik_create would
        std::vector<uint64_t> h_cp((size_t)dx->n + 1);
        std::vector<uint32_t> h_row((size_t)dx->nnz);
        std::vector<float> h_val;
        POLEE_TRY(dx->cp.download(ctx, h_cp.data(), h_cp.size()));
        const float *vals = nullptr;
        if (dx->nnz) {
            POLEE_TRY(dx->rowval.download(ctx, h_row.data(), h_row.size()));
            if (dx->nzval.p) {
                h_val.resize((size_t)dx->nnz);
                POLEE_TRY(dx->nzval.download(ctx, h_val.data(), h_val.size()));
                vals = h_val.data();
            } else {
                vals = nzval;  // (values that were to go up late never did: the caller's host array is the source)
            }
        }
        return polee_loglik_create_impl(ctx, dx->m, dx->n, h_cp.data(), 8, h_row.data(), vals, ks, out);
    });
}

polee_status polee_loglik_get_info(const polee_loglik *ll, polee_loglik_info *info)
{
    return entry(ll, "polee_loglik_get_info", [&](polee_ctx *ctx) -> polee_status {
        if (!info) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_loglik_get_info: null argument");
        const PsellHost &h = ll->host;
        info->m = ll->m;
        info->n = ll->n;
        info->nnz = ll->nnz;
        info->num_slices = h.num_slices;
        info->num_tiles = h.num_tiles;
        info->padded_nnz = h.padded_nnz;
        info->stream_bytes = (int64_t)(ll->d_data.n + 4 * (ll->d_slice_off.n + ll->d_tile_slice.n + ll->d_tile_dict.n +
                                                            ll->d_dict.n + ll->d_slice_ks.n + ll->d_csr_rowptr.n + ll->d_csr_col.n +
                                                            ll->d_csr_val.n + ll->d_csr_ks.n));
        info->device_bytes = info->stream_bytes;
        info->num_empty_rows = h.empty_rows;
        info->max_row_nnz = h.max_row;
        info->max_tile_cols = h.max_tile_cols;
        const int64_t tiles[PSELL_NSTREAMS] = {h.num_tiles_a1, h.num_tiles_a1m - h.num_tiles_a1, h.num_tiles_a2 - h.num_tiles_a1m,
                                               h.num_tiles_a - h.num_tiles_a2, h.num_tiles_s - h.num_tiles_a, h.num_tiles - h.num_tiles_s, 0};
        for (int i = 0; i < 8; ++i) info->stream_rows[i] = info->stream_nnz[i] = info->stream_tiles[i] = info->stream_bytes_hbm[i] = 0;
        for (int i = 0; i < PSELL_NSTREAMS; ++i) {
            info->stream_rows[i] = h.stream_rows[i];
            info->stream_nnz[i] = h.stream_nnz[i];
            info->stream_tiles[i] = tiles[i];
            info->stream_bytes_hbm[i] = h.stream_bytes[i];
        }
        info->dict_entries = ll->dict_len;
        return POLEE_OK;
    });
}

}  // extern "C"
