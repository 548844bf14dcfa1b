// The persistent streaming kernel of the sparse pass (loglik_stream_kernel) and its building blocks: LDS-DMA, the waves' rings,
// the four slice loops.  Device code of ONE translation unit: included by loglik.hip only (the Makefile compiles that file with
// backend options chosen for this kernel).
#pragma once
#include "loglik_internal.hpp"
#include "wave.hpp"

#include <type_traits>

namespace polee {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
// LDS by 32-bit address.  Every LDS access of the slice loops names its address space: a generic (flat) access would count
// against vmcnt and break the rings' counted waits.
typedef const __attribute__((address_space(3))) float *lds_cfp;
typedef __attribute__((address_space(3))) float *lds_fp;
typedef const __attribute__((address_space(3))) f32x2 *lds_cf2p;
typedef const __attribute__((address_space(3))) uint16_t *lds_cu16p;
__device__ inline float lds_f(uint32_t a) { return *reinterpret_cast<lds_cfp>((uintptr_t)a); }

template <int CTRL, int ROW_MASK>
__device__ inline float dpp_mov0(float v)  // lanes without a source (or in masked-off rows) read 0
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, true));
}

__device__ inline float fast_weight(float ksv, float s)
{
    // ks / s with v_rcp_f32 (1 ulp): well inside the 1e-4 budget, 10x fewer instructions than a division
    return s > 0.0f ? ksv * __builtin_amdgcn_rcpf(s) : 0.0f;  // padded lanes (and empty rows) have s = 0
}
// Row sums of the matrix-core path start from FLT_MIN instead of 0: a padded lane (no fragment: only zero values) then
// has s = FLT_MIN and a finite weight 1 / FLT_MIN, which multiplies zeros; a real row sum (values >= 1e-12, x >= 1e-16:
// s >= 1e-28) is unchanged by the addend, bit for bit.  The weight is then one v_rcp_f32, no compare or select.
constexpr float ROWSUM_FLOOR = 1.17549435e-38f;

// Sum of the logs of a lane's row sums WITHOUT a logarithm in the slice loop.  log s = exponent(s) ln 2 + log mantissa(s), so
// a lane keeps the PRODUCT of the mantissas (brought back into [0.5, 1) at every step) and the SUM of the exponents -- two
// v_frexp pairs, a multiply and two integer adds per row sum, no float64 -- and takes one logarithm when its share of the
// tile is done.  The mantissa product is rounded to float32 at every step: a relative 6e-8 per factor, i.e. an absolute
// ~1e-6 on the log of a lane's ~100 row sums, against log-likelihoods of 1e6 .. 1e9.  (The float64 log per row sum that
// stood here kept ~30 registers live inside the loop: with the masked streams in the same kernel the instances that
// return lp spilled, and a spill's reload drains the LDS-DMA ring -- the pass took 1.40 ms instead of 0.25.)
struct LogAcc {
    float m;  // in [0.5, 1)
    int e;
    __device__ inline void init()
    {
        m = 0.5f;
        e = 1;
    }
    __device__ inline void mul(float s, bool valid)  // *= s (valid) or *= 1
    {
        const float sv = valid ? s : 1.0f;
        const float p = m * __builtin_amdgcn_frexp_mantf(sv);
        m = __builtin_amdgcn_frexp_mantf(p);
        e += __builtin_amdgcn_frexp_expf(sv) + __builtin_amdgcn_frexp_expf(p);
    }
    // (the mantissa's log with the hardware log2 -- an absolute 1e-7, once per lane and tile: no float64 logarithm, with its
    // thirty live registers, anywhere in the kernel)
    __device__ inline double log_value() const { return ((double)e + (double)__builtin_amdgcn_logf(m)) * 0.693147180559945309417; }
};
// multiplicities: ks log s with the hardware log2 (1 ulp of float32), summed in float64; x ln 2 at the end
__device__ inline double ks_log2(float ksv, float s) { return (double)(ksv * __builtin_amdgcn_logf(s)); }

// arguments of a pass's kernels (the per-tile kernel of loglik.hip takes them too)
struct PsellArgs {
    const uint8_t *data;
    const uint32_t *slice_off, *tile_slice, *tile_dict, *dict;
    const float *slice_ks;
    const float *x;
    float *g;
    double *lp;
    int lcap;
    int tiles_a;  // tiles [0, tiles_a) use the compact uniform slice layouts
    // the persistent streaming kernel
    int tiles_a1;           // tiles [0, tiles_a1): stream A1 (dense narrow), [tiles_a1, tiles_a1m): A1M (masked narrow),
    int tiles_a1m, tiles_a2;  // [tiles_a1m, tiles_a2): A2 (dense wide), [tiles_a2, tiles_a): A2M (masked wide)
    int tiles_s;              // [tiles_a, tiles_s): BN (mixed narrow); the persistent launch's share ends here
    const float *xwin;      // x window of every tile: xwin[e * K + k] = x[dict[e]][k]
    const PosDesc *sched;   // [rounds + 1][grid] static schedule, POS_NONE-terminated columns
    // dynamic schedule (the default; the deterministic mode keeps the static one only when lp is wanted): the tiles in descending order of their
    // cost, POS_NONE behind them; workgroup b starts with positions b, b + G, b + 2 G and draws every further position
    // from the counter dyn_ctr[0] (+ 3 G).  The counter is NEVER reset: a launch makes exactly one draw per position of the list
    // (a workgroup draws once per tile it takes), so the next launch's draws start at dyn_base + positions -- the host keeps
    // dyn_base (round 5: the last workgroup used to reset the counter behind an acquire-release arrival count; that fence --
    // an L2 write-back and invalidate per WORKGROUP, 1 024 per launch -- cost 25 us of a 250 us pass, see launch_stream)
    const PosDesc *sched_dyn;
    unsigned int *dyn_ctr;
    unsigned int dyn_base;
    unsigned int dyn_last;  // the list's last (POS_NONE) slot: a draw is clamped to it, so that a counter that has fallen out of step
                            // with the host's base (an asynchronous fault, two evaluations of one handle at once) ends the
                            // workgroup's walk instead of indexing past the list
    // deterministic mode: every tile's window is stored (not added) and a second kernel sums the windows of a transcript
    float *gwin;            // [dict entries][K], laid out like xwin
    double *lpwin;          // [grid][K] per-workgroup log-likelihood sums, then [stream B's tiles][K] (lp_slot0 on)
    int lp_slot0;
};

// ---- the uniform streams in ONE persistent launch --------------------------------------------------------------
// A uniform slice holds up to 64 fragments (one per lane) that share ONE transcript set (c_0..c_{w-1}); runs of
// consecutive slices with the same set are marked by the builder.  For such a slice V[t][r] (w x 64):
//     S[r][k]  = sum_t V[t][r] x[c_t][k]          (phase 1)
//     G[t][k] += sum_r V[t][r] ks_r / S[r][k]     (phase 2 = the transpose of phase 1)
// Both run on the matrix cores (exact-f32 MFMA), the weights never leave the registers, and the partial G stays
// in registers for the whole run; it is added to the tile's LDS window when the run ends.
//
// Streaming: each wave owns a contiguous byte range of the tile's slice stream and pulls it through a private LDS
// ring with `global_load_lds_dwordx4` (1 KiB per wave-instruction, no VGPR destination), ring-size ahead; HBM sees
// every byte of X exactly once.
//
// Persistence: the grid is (workgroups per CU) x (CUs); every workgroup walks its own column of a static schedule
// (sched[pos], pos = block + round * grid: tiles dealt in snake order of their cost, small tiles spread between the
// large ones).  While a tile streams, everything the NEXT tile needs arrives in the background by LDS-DMA: its x
// window (one contiguous piece of xwin, gathered once per pass by xwin_gather_kernel), the transcript ids of its
// dictionary (for the flush) and the slice offsets of each wave's share; a wave that has finished its slices
// starts the next tile's ring before the workgroup's barrier.  A tile therefore has no dependent global latency in
// front of its first slice; the counted `s_waitcnt vmcnt(N)` of the slice loop account for these extra operations.
#ifndef POLEE_DMA_POLICY
#define POLEE_DMA_POLICY " nt"  // X is read once per pass: non-temporal keeps it from evicting x / g lines
#endif
// a wave-uniform pointer the compiler cannot prove uniform, as an SGPR pair
__device__ inline const void *uniform_ptr(const void *p)
{
    const uint64_t a = (uint64_t)(uintptr_t)p;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));
    return (const void *)(uintptr_t)(((uint64_t)hi << 32) | lo);
}
// LDS-DMA forms: wave-uniform 64-bit base in SGPRs + a 32-bit byte offset per lane; the LDS destination is
// M0 + lane * (bytes per lane).  The leading s_nop 4 covers a base that has just come out of v_readfirstlane
// (VALU-written SGPR -> VMEM read: 5 wait states, which the compiler does not insert for an asm statement).  (M0 is not restored, and it
// cannot be declared clobbered: hipcc treats M0 as a reserved register and warns that such a clobber is not honoured.
// Nothing else in these kernels uses it -- LDS instructions on gfx9 do not, there is no movrel / sendmsg -- and the base /
// offset registers are not rewritten per piece.)
#ifdef POLEE_DMA_BUILTIN
// A/B build (`make dmabuiltin`): the LDS-DMA through the compiler's builtin, which models M0 (no
// unmodelled write) but takes a per-lane 64-bit global address instead of SGPR base + 32-bit lane offset.
__device__ inline void dma_builtin(const void *base_uniform, uint32_t voff, uint32_t lds_dst_any, int bytes16)
{
    typedef __attribute__((address_space(3))) void *lds_vp;
    typedef const __attribute__((address_space(1))) void *glb_vp;
    const uint32_t lds_dst = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_dst_any);
    glb_vp src = (glb_vp)(reinterpret_cast<const char *>(base_uniform) + voff);
    if (bytes16)
        __builtin_amdgcn_global_load_lds(src, (lds_vp)(uintptr_t)lds_dst, 16, 0, 0);
    else
        __builtin_amdgcn_global_load_lds(src, (lds_vp)(uintptr_t)lds_dst, 4, 0, 0);
}
__device__ inline void dma_1k(const void *b, uint32_t v, uint32_t l) { dma_builtin(b, v, l, 1); }
__device__ inline void dma_1k_keep(const void *b, uint32_t v, uint32_t l) { dma_builtin(b, v, l, 1); }
__device__ inline void dma_1k_next(const void *b, uint32_t v, uint32_t l) { dma_builtin(b, v, l, 1); }
__device__ inline void dma_256(const void *b, uint32_t v, uint32_t l) { dma_builtin(b, v, l, 0); }
#else
__device__ inline void dma_1k(const void *base_uniform, uint32_t voff, uint32_t lds_dst_any)
{
    const uint32_t lds_dst = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_dst_any);
    asm volatile("s_nop 4\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %0" POLEE_DMA_POLICY
                 :
                 : "s"(base_uniform), "v"(voff), "s"(lds_dst)
                 : "memory");
}
// A further piece of a burst whose first piece went out with dma_1k in the same straight line: the base is the same SGPR pair
// (nothing rewrites it between the pieces: the lane offset moves, a vector register), so the wait states have been served and
// only M0 changes.  `lds_dst` must be wave-uniform as written.
__device__ inline void dma_1k_next(const void *base_uniform, uint32_t voff, uint32_t lds_dst)
{
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %0" POLEE_DMA_POLICY
                 :
                 : "s"(base_uniform), "v"(voff), "s"(lds_dst)
                 : "memory");
}
// the same with the default cache policy (x windows: written by the previous kernel)
__device__ inline void dma_1k_keep(const void *base_uniform, uint32_t voff, uint32_t lds_dst_any)
{
    const uint32_t lds_dst = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_dst_any);
    asm volatile("s_nop 4\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %0" : : "s"(base_uniform), "v"(voff), "s"(lds_dst) : "memory");
}
// 4 bytes per lane: 64 dwords -> 256 contiguous LDS bytes
__device__ inline void dma_256(const void *base_uniform, uint32_t voff, uint32_t lds_dst_any)
{
    const uint32_t lds_dst = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_dst_any);
    asm volatile("s_nop 4\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, %0" : : "s"(base_uniform), "v"(voff), "s"(lds_dst) : "memory");
}
#endif
__device__ inline uint32_t lds_addr(const void *p)
{
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)(uintptr_t)(__attribute__((address_space(3))) const char *)p);
}

// waits until at most `allowed` of this wave's vector-memory operations are outstanding (rounded down
// to an encodable step: waiting for fewer outstanding operations is always safe)
__device__ inline void wait_vm_outstanding(int allowed)
{
    if (allowed >= 8) {
        if (allowed >= 14)
            asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
        else if (allowed >= 12)
            asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        else if (allowed >= 10)
            asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
        else
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else if (allowed >= 4) {
        if (allowed >= 7)
            asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
        else if (allowed >= 6)
            asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else if (allowed >= 5)
            asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
        if (allowed >= 3)
            asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        else if (allowed >= 2)
            asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else if (allowed >= 1)
            asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
        else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
}

// The slice loops of the matrix-core streams: with the whole ring requested ahead, `allowed` is the ring's seven pieces
// minus the pieces the slice touches -- 3 .. 5 for sets of 4 .. 12 transcripts -- so those values are tested first (one or
// two scalar compares instead of the ladder's four or five); everything else takes the ladder.
__device__ inline void wait_vm_steady(int allowed)
{
    if (allowed == 4)
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if (allowed == 5)
        asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else if (allowed == 3)
        asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else
        wait_vm_outstanding(allowed);
}

// This lane's index in its wave, computed where it is used (two instructions): a lane index kept in a register across
// the tile loop is spilled under the slice loop's register pressure, and its reload comes with an s_waitcnt vmcnt(0) that
// drains the LDS-DMA ring which has just been started.
__device__ inline int wave_lane()
{
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// workgroup barrier for LDS hand-offs only: waits for this wave's LDS operations, not for its vector-memory queue
// (__syncthreads() would drain the LDS-DMA ring that has just been started for the next tile)
__device__ inline void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

#ifdef POLEE_STAMPS
// diagnostic build only: where does a wave of the streaming kernel spend its cycles?
__device__ unsigned long long g_stamps[24];
__device__ unsigned long long g_stamps_wave[4][24];  // the same per wave index of the workgroup (wave 0 carries the schedule DMA and the ticket)
constexpr int NSTAMP = 17;
struct Stamps {
    unsigned long long acc[NSTAMP];
    unsigned long long last;
    __device__ inline Stamps() : acc{}, last(__builtin_amdgcn_s_memtime()) {}
    __device__ inline void mark(int i)  // the cycles since the previous mark go to entry i
    {
        const unsigned long long now = __builtin_amdgcn_s_memtime();
        acc[i] += now - last;
        last = now;
    }
};
#else
struct Stamps {  // the production build: nothing
    __device__ inline void mark(int) {}
};
#endif
#define STAMP(i) st.mark(i)  // (the kernel and every slice loop call their Stamps `st`)
#ifdef POLEE_TILE_CYCLES
// second diagnostic build (cheap: one clock read per tile): how long does every tile / every workgroup take?
__device__ unsigned long long g_tile_cycles[1 << 17];  // per tile: wave 0's time from the previous tile's end to this tile's end
__device__ unsigned long long g_wg_cycles[4096];       // per workgroup: wave 0's time in the kernel
#endif

// what a wave knows about its share of the current uniform tile
struct WaveStream {
    uint32_t ent;         // slice offset (+ flags) of slice sb + lane, one per lane
    int nsl;              // slices owned by this wave
    int npieces;          // 1 KiB pieces of its byte range
    int issued;           // pieces requested so far
    uint32_t slot;        // byte offset, inside the ring, of the slot the next piece goes to
    int primed;           // pieces requested before the tile's loop started
    const uint8_t *gsrc;  // start of the byte range (wave-uniform)
};

// Requests the pieces [issued, target) of a wave's byte range, piece after piece into consecutive ring slots.  Everything here
// is wave-uniform and the caller holds it in scalar registers: `gsrc`, the START of the range -- an SGPR pair that is not
// advanced: a piece's position travels in the lanes' 32-bit byte offsets, one vector add per piece (a wave's share of a tile is
// far below 4 GiB), so the wait states between a freshly read SGPR base and the first vector-memory instruction that uses it
// are paid once per burst (dma_1k), not once per piece (dma_1k_next) --, the piece counter, and the ring offset of the next slot.
// `lane_word`: ring_lds + 4 x lane where the caller holds that lane constant in a register anyway (the lanes' offsets are then one
// shift-and-add on it per burst), 0 where it does not (the lane index is computed here: wave_lane).
template <uint32_t RB, bool LANE_WORD = false>
__device__ inline void ring_issue(const uint8_t *gsrc, uint32_t ring_lds, int &issued, uint32_t &slot, int target, uint32_t lane_word = 0u)
{
    if (issued >= target) return;
    uint32_t voff = LANE_WORD ? (lane_word << 2) + ((uint32_t)issued * 1024u - 4u * ring_lds) : (uint32_t)wave_lane() * 16u + (uint32_t)issued * 1024u;
    dma_1k(gsrc, voff, ring_lds + slot);
    for (;;) {
        slot = slot + 1024u == RB ? 0u : slot + 1024u;
        if (++issued >= target) break;
        voff += 1024u;
        dma_1k_next(gsrc, voff, ring_lds + slot);
    }
}
// the same on a WaveStream (the loops that do not keep the counters in locals of their own)
template <uint32_t RB>
__device__ inline void ring_refill(WaveStream &ws, uint32_t ring_lds, int target)
{
    // (wave-uniform counters: say so, or the loop is compiled as a divergent loop on vector registers)
    int issued = __builtin_amdgcn_readfirstlane(ws.issued);
    uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)ws.slot);
    ring_issue<RB>(reinterpret_cast<const uint8_t *>(uniform_ptr(ws.gsrc)), ring_lds, issued, slot, __builtin_amdgcn_readfirstlane(target));
    ws.issued = issued;
    ws.slot = slot;
}
template <uint32_t RB>
__device__ inline uint32_t wrap_u(uint32_t a)  // uniform ring offset a < 2 RB
{
    a = (uint32_t)__builtin_amdgcn_readfirstlane((int)a);
    return a >= RB ? a - RB : a;
}

// A wave's ring while it walks the slices of a tile: the tail, the waits for bytes behind it and their release.  The wave-uniform
// counters and the range's start are loaded once from the WaveStream and stay in scalar registers for the whole tile (ring_issue).
// `extras` = vector-memory operations issued AFTER the primed ring pieces and before the first refill (the previous tile's flush,
// the next tile's prefetch): they are younger than the primed pieces and older than every other piece, so only waits for primed
// pieces have to allow for them.
template <uint32_t RB, bool LANE_WORD = false>
struct RingCursor {
    static constexpr int RP = (int)(RB / 1024u);
    const uint32_t ring_lds;
    const uint32_t lane_word;  // (LANE_WORD) see ring_issue
    const int extras;
    int issued;
    uint32_t slot;
    const int primed, npieces;
    const uint8_t *const gsrc;
    uint32_t pos = 0;    // byte offset of the ring's tail inside this wave's range
    uint32_t pos_r = 0;  // pos modulo the ring size
    __device__ inline RingCursor(const WaveStream &ws, uint32_t ring_lds_, int extras_, uint32_t lane_word_ = 0u)
        : ring_lds(ring_lds_), lane_word(lane_word_), extras(extras_), issued(__builtin_amdgcn_readfirstlane(ws.issued)),
          slot((uint32_t)__builtin_amdgcn_readfirstlane((int)ws.slot)), primed(__builtin_amdgcn_readfirstlane(ws.primed)),
          npieces(__builtin_amdgcn_readfirstlane(ws.npieces)), gsrc(reinterpret_cast<const uint8_t *>(uniform_ptr(ws.gsrc)))
    {
    }
    // (wave-uniform: said explicitly, or the waits' ladders are compiled with vector compares and exec masks)
    __device__ inline int allowed(int need) const { return __builtin_amdgcn_readfirstlane(issued - need + (need <= primed ? extras : 0)); }
    __device__ inline void wait_for(uint32_t upto)  // bytes [pos, pos + upto) of the wave's range must have landed
    {
        const int need = (int)((pos + upto + 1023u) >> 10);
        if (issued < need) ring_issue<RB, LANE_WORD>(gsrc, ring_lds, issued, slot, need, lane_word);  // (only with a shortened look-ahead: experiments)
        wait_vm_outstanding(allowed(need));
    }
    __device__ inline void wait_for_steady(uint32_t upto)  // the same with the whole ring requested ahead (wait_vm_steady)
    {
        wait_vm_steady(allowed((int)((pos + upto + 1023u) >> 10)));
    }
    __device__ inline void advance(uint32_t nbytes)  // the tail moves on; the DMA for what follows goes out
    {
        pos += nbytes;
        pos_r += nbytes;
        pos_r = pos_r >= RB ? pos_r - RB : pos_r;
        ring_issue<RB, LANE_WORD>(gsrc, ring_lds, issued, slot, min(npieces, (int)(pos >> 10) + RP), lane_word);
    }
    __device__ inline void release(uint32_t nbytes)  // the first nbytes behind the tail are consumed
    {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        advance(nbytes);
    }
};
// The same waits and release with the counters left on the WaveStream (ring_refill): the mixed and the wide masked loop, which
// keep `pos` / `pos_r` (the tail inside the wave's range, and modulo the ring size) in locals of their own
template <uint32_t RB>
__device__ inline void stream_wait_for(WaveStream &ws, uint32_t ring_lds, uint32_t pos, uint32_t upto, int extras)
{
    const int need = (int)((pos + upto + 1023u) >> 10);
    if (ws.issued < need) ring_refill<RB>(ws, ring_lds, need);
    int allowed = ws.issued - need + (need <= ws.primed ? extras : 0);
    wait_vm_outstanding(__builtin_amdgcn_readfirstlane(allowed));
}
template <uint32_t RB>
__device__ inline void stream_advance(WaveStream &ws, uint32_t ring_lds, uint32_t &pos, uint32_t &pos_r, uint32_t nbytes)
{
    pos += nbytes;
    pos_r += nbytes;
    pos_r = pos_r >= RB ? pos_r - RB : pos_r;
    ring_refill<RB>(ws, ring_lds, min(ws.npieces, (int)(pos >> 10) + (int)(RB / 1024u)));
}
// every operand of a slice is in registers: its ring bytes are free, the DMA for the pieces behind it (`advance`: the loop's
// ring moves its tail on) goes out before the (rest of the) matrix phases
template <class Advance>
__device__ inline void slice_consumed(Advance &&advance, Stamps &st, int dbg)
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    STAMP(11);  // operand reads landed
    advance();
    STAMP(6);  // refill
    if (!(dbg & 16)) __builtin_amdgcn_s_setprio(0);
}

// A slice's entry: e0 = its offset word (128-byte units in the low bits, the flags on top), e1 = the next slice's
// (the slice loops below spell out "rows from units" and kind_of by hand; the format they restate is psell_slice.hpp's)
struct SliceEntry {
    uint32_t units, bytes;
    int flags;  // bit 1: the slice continues the previous one's transcript set
};
__device__ inline SliceEntry slice_entry(uint32_t e0, uint32_t e1)
{
    const uint32_t units = (e1 & PSELL_OFF_MASK) - (e0 & PSELL_OFF_MASK);
    return SliceEntry{units, units * 128u, (int)(e0 >> 30)};
}

// The slice loop of one wave over its share of a tile of the WIDE stream (A2: transcript sets of 17..32; 16 x 16 x 4 matrix
// tiles -- the narrow stream has its own loop, narrow_stream below).  `extras`: see RingCursor.
//
// Round 5: ALL FOUR waves of the workgroup work on a wide tile, each with the narrow streams' 7 KiB ring (until round 4 two
// waves with 14 KiB rings did, the other two waited at the tile's barrier: 15 % of all wave time on the SURVEY 8(d)
// generator, 40 % on inputs of wide sets).  A wide slice is up to 2 + 32 rows of 256 bytes and does not fit such a ring
// together with any look-ahead, so it passes through in TWO STAGES:
//   stage A   header + transcripts 0..15 (4 352 bytes): the phase-1 operands of steps 0..3 AND the phase-2 operands of the
//             first 16-row tile are read into registers (32), the bytes are released, the DMA for what follows goes out,
//             phase 1 runs over the first sixteen transcripts;
//   stage B   transcripts 16..w-1 (+ the multiplicities): phase 1 over them, the weights, the phase-2 operands of the
//             second tile (in the registers the phase-1 operands have left), release, then both tiles' phase 2.
// At any time the ring holds at most 4 352 bytes of the current slice + the look-ahead.
template <int K, uint32_t RB, bool WANT_LP, bool HAS_KS>
__device__ inline void wide_stream(WaveStream &ws, const char *ring, int extras, const float *xw, float *gw, double &lpacc, int dbg, Stamps &st)
{
    constexpr uint32_t STAGE_A = 256u + 16u * 256u;  // header + sixteen rows
    static_assert(STAGE_A + 2046u <= RB && (PSELL_WIDE_MAX - 16 + 1) * 256u + 2046u <= RB, "a stage of a wide slice (+ ks row) must fit the ring");
    // (computed here, opaquely: the lane constants below are then recomputed per tile -- a few dozen instructions --
    // instead of being hoisted out of the kernel's tile loop, kept alive across it and spilled)
    const int lane = wave_lane();
    const uint32_t ring_lds = lds_addr(ring);

    // lane l = (tt = l & 15, q = l >> 4).  A slice is a (w x 64) block V[t][r]:
    //   phase 1   S[r][k] = sum_t V[t][r] x[c_t][k]      M = r (4 tiles: tile e holds rows 4 i + e), N = k, inner = t
    //       A[i][kk=q] = V[4 step + q][4 i + e]  -- one 16-byte LDS read per step feeds the 4 row tiles
    //       B[kk=q][tt] = x[c_{4 step + q}][tt]  -- constant over a run, kept in registers (xq)
    //       D1[e]: lane (tt, q), register v  =  S[16 q + 4 v + e][tt]
    //   weights   W = ks / S, in place (v_rcp_f32)
    //   phase 2   G[t][k] += sum_r V[t][r] W[k][r]      M = t, N = k, inner = r = 16 q + (0..15)
    //       A[tt][kk=q] = V[16 mt + tt][16 q + 4 j + e]   -- four 16-byte LDS reads per 16-row tile mt
    //       B[kk=q][tt] = W[tt][16 q + 4 j + e]   = D1[e][j] of THIS lane: the weights never leave the registers
    //       D2 (rows 4 q + v, column tt) stays in registers for the whole run of slices sharing the set.
    // Rows are stored ROTATED (element r of row t at position (r + 4 t) & 63) so that the 16 lanes of every
    // 16-byte read hit 16 different bank groups.  Columns tt >= K are padding (B = 0 there).
    constexpr int NT = 2;  // 16-row tiles of transcripts (phase 2)
    constexpr int NS = 8;  // steps of 4 transcripts (phase 1)
    const int tt = lane & 15, q = lane >> 4;
    f32x4 acc0[NT], acc1[NT];  // two accumulation chains per tile (dependent MFMA latency 40 > issue 32)
    uint2 colq[NT];            // tile-local ids of transcripts 16 mt + 4 q + (0..3) of the current run, 16 bit each
    float xq[NS];              // x[c_{4 step + q}][tt] of the current run
#pragma unroll
    for (int mt = 0; mt < NT; ++mt) {
        acc0[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        acc1[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        colq[mt] = make_uint2(0u, 0u);
    }
#pragma unroll
    for (int sp = 0; sp < NS; ++sp) xq[sp] = 0.0f;
    int pend_w = 0;  // transcripts of the current run (0: no run open)
    LogAcc lpl;       // (WANT_LP) log of the product of this lane's row sums; with multiplicities: lp2 = sum ks log2 s
    lpl.init();
    double lp2 = 0.0;
    auto flush = [&]() {
#pragma unroll
        for (int mt = 0; mt < NT; ++mt) {
            if (16 * mt < pend_w) {
                const f32x4 sum = acc0[mt] + acc1[mt];
                const unsigned cid[4] = {colq[mt].x & 0xffffu, colq[mt].x >> 16, colq[mt].y & 0xffffu, colq[mt].y >> 16};
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (tt < K && 16 * mt + 4 * q + v < pend_w && sum[v] != 0.0f && !(dbg & 2))
                        atomicAdd(gw + cid[v] * K + tt, sum[v]);
                acc0[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
                acc1[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        pend_w = 0;
    };

    // Operand addresses.  A slice starts at a multiple of 256 bytes and the ring holds whole 256-byte rows, so a row never
    // straddles the ring's end: address = ring + wrap(stage base + 256 x row) + (offset inside the row).  Rows t >= w of a
    // step (B = 0 there) or of the second tile (their D2 rows are never used) read whatever follows the slice in the ring --
    // stream bytes or the zeros the ring was initialised with, always finite.
    const uint32_t q256 = 256u * (uint32_t)q;
    auto k2f = [&](int sp) -> uint32_t { return ring_lds + (uint32_t)((tt + 4 * sp + q) & 15) * 16u; };  // phase 1, step sp: row 4 sp + q, chunk (tt + row) & 15
    auto c2f = [&](int mt, int j) -> uint32_t { return ring_lds + (uint32_t)((4 * q + j + 16 * mt + tt) & 15) * 16u; };  // phase 2, tile mt: row 16 mt + tt
    auto lds_f4 = [](uint32_t a) -> f32x4 {
        return *reinterpret_cast<const __attribute__((address_space(3))) f32x4 *>((uintptr_t)a);
    };
    auto wrap = [&](uint32_t a) -> uint32_t { return min(a, a - RB); };  // a < 2 RB: a mod RB (unsigned wrap-around)

    RingCursor<RB> rc(ws, ring_lds, extras);  // (the tail stands at a slice start, or STAGE_A behind one)
    uint32_t e_next = (uint32_t)__builtin_amdgcn_readlane((int)ws.ent, 0);  // (a slice's end is the next one's start: one lane read per slice)
    for (int si = 0; si < ws.nsl; ++si) {
        const uint32_t e0 = e_next;
        const uint32_t e1 = (uint32_t)__builtin_amdgcn_readlane((int)ws.ent, si + 1);
        e_next = e1;
        const SliceEntry se = slice_entry(e0, e1);
        const int flags = se.flags;
        const int w = (int)(se.units / 2u) - 1 - (HAS_KS ? 1 : 0);  // 256-byte header (column ids) + w rows of 64 values (+ ks row)
        const uint32_t bytes = se.bytes;
        const bool two = w > 16;  // (always, as the builders fill this stream; a narrower slice passes in one stage)
        if (!(dbg & 16)) __builtin_amdgcn_s_setprio(3);  // the short non-matrix sections of a slice win the issue arbitration
        STAMP(1);  // slice bookkeeping
        rc.wait_for(two ? STAGE_A : bytes);
        STAMP(2);  // waiting for the DMA
        if (pend_w != 0 && !(flags & 2)) flush();
        if (pend_w == 0) {  // a new run: the tile-local ids of its transcripts and their x rows (all in the header)
            const char *hdr = ring + rc.pos_r;
#pragma unroll
            for (int mt = 0; mt < NT; ++mt) colq[mt] = *reinterpret_cast<const uint2 *>(hdr + 32 * mt + 8 * q);
            int cl[NS];
#pragma unroll
            for (int sp = 0; sp < NS; ++sp) cl[sp] = *reinterpret_cast<const uint16_t *>(hdr + 2 * min(4 * sp + q, w - 1));
#pragma unroll
            for (int sp = 0; sp < NS; ++sp) {
                const float xv = xw[cl[sp] * K + min(tt, K - 1)];
                xq[sp] = (tt < K && 4 * sp + q < w) ? xv : 0.0f;
            }
        }
        STAMP(3);  // run change: flush + column lookup

        f32x4 d1[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) d1[e] = f32x4{ROWSUM_FLOOR, ROWSUM_FLOOR, ROWSUM_FLOOR, ROWSUM_FLOOR};
        f32x4 av1[4], av2a[4], av2b[4];
        auto phase1 = [&](int st0) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (4 * (st0 + u) < w) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) d1[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(av1[u][e], xq[st0 + u], d1[e], 0, 0, 0);
                }
            }
        };
        // ---- stage A: transcripts 0..15
        {
            const uint32_t rows = rc.pos_r + 256u;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (4 * u < w) av1[u] = lds_f4(wrap(rows + 1024u * (uint32_t)u + q256) + k2f(u));
            const uint32_t row = wrap(rows + 256u * (uint32_t)tt);
#pragma unroll
            for (int j = 0; j < 4; ++j) av2a[j] = lds_f4(row + c2f(0, j));
        }
        // weights, in place: d1[e][v] belongs to fragment r = 16 q + 4 v + e, draw tt.  With multiplicities (the slice's last row:
        // ks of fragments 16 q + 4 v + (0..3) at `kr`) they are read four at a time, so the weights come BEFORE the release.
        auto weights = [&](uint32_t kr) {
            if (HAS_KS) {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const f32x4 kv = lds_f4(ring_lds + kr + 16u * (uint32_t)v);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float sv = d1[e][v];
                        if (WANT_LP && sv > 2.0f * ROWSUM_FLOOR) lp2 += ks_log2(kv[e], sv);
                        d1[e][v] = kv[e] * __builtin_amdgcn_rcpf(sv);  // (padded lanes: ks = 0)
                    }
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const float sv = d1[e][v];
                        if (WANT_LP) lpl.mul(sv, sv > 2.0f * ROWSUM_FLOOR);
                        d1[e][v] = __builtin_amdgcn_rcpf(sv);
                    }
            }
        };
        if (two) {
            rc.release(STAGE_A);
            STAMP(6);  // refill
            if (!(dbg & 16)) __builtin_amdgcn_s_setprio(0);
            phase1(0);
            // ---- stage B: transcripts 16..w-1; the tail now stands at row 16
            if (!(dbg & 16)) __builtin_amdgcn_s_setprio(3);
            STAMP(14);  // phase 1 MFMAs
            rc.wait_for(bytes - STAGE_A);
            STAMP(2);  // waiting for the DMA
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (4 * (4 + u) < w) av1[u] = lds_f4(wrap(rc.pos_r + 1024u * (uint32_t)u + q256) + k2f(4 + u));
            if (!(dbg & 16)) __builtin_amdgcn_s_setprio(0);
            phase1(4);
            // the second tile's phase-2 operands (rows t >= w: whatever lies there), in the registers the phase-1 operands have left
            const uint32_t row = wrap(rc.pos_r + 256u * (uint32_t)tt);
#pragma unroll
            for (int j = 0; j < 4; ++j) av2b[j] = lds_f4(row + c2f(1, j));
            if (HAS_KS) weights(wrap(rc.pos_r + 256u * (uint32_t)(w - 16)) + 64u * (uint32_t)q);
            rc.release(bytes - STAGE_A);
            STAMP(6);  // refill
            if (!HAS_KS) weights(0u);
        } else if (HAS_KS) {
            if (!(dbg & 16)) __builtin_amdgcn_s_setprio(0);
            phase1(0);
            weights(wrap(rc.pos_r + 256u + 256u * (uint32_t)w) + 64u * (uint32_t)q);
            rc.release(bytes);
            STAMP(6);  // refill
        } else {
            rc.release(bytes);
            STAMP(6);  // refill
            if (!(dbg & 16)) __builtin_amdgcn_s_setprio(0);
            phase1(0);
            weights(0u);
        }
        STAMP(4);  // phase 1 + weights
        if (!(dbg & 2)) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc0[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av2a[j][0], d1[0][j], acc0[0], 0, 0, 0);
                acc1[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av2a[j][1], d1[1][j], acc1[0], 0, 0, 0);
                acc0[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av2a[j][2], d1[2][j], acc0[0], 0, 0, 0);
                acc1[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av2a[j][3], d1[3][j], acc1[0], 0, 0, 0);
            }
            if (two) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc0[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av2b[j][0], d1[0][j], acc0[1], 0, 0, 0);
                    acc1[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av2b[j][1], d1[1][j], acc1[1], 0, 0, 0);
                    acc0[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av2b[j][2], d1[2][j], acc0[1], 0, 0, 0);
                    acc1[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av2b[j][3], d1[3][j], acc1[1], 0, 0, 0);
                }
            }
        }
        pend_w = w;
        STAMP(5);  // phase 2
    }
    if (pend_w != 0) flush();
    if (WANT_LP) lpacc += HAS_KS ? lp2 * 0.693147180559945309417 : lpl.log_value();
}


// ---- the slice loop of the narrow stream (transcript sets of <= 16): batched outer products ---------------------------
// With K <= 8 draws the 16-column MFMA tile of wide_stream is at most half used.  v_mfma_f32_4x4x1_16b_f32 computes
// sixteen independent 4 x 4 outer products D[b][i][j] += A[b][i] B[b][j] (A in lane 4 b + i, B in lane 4 b + j, D in
// register i of lane 4 b + j) in 8 cycles, a quarter of the 16 x 16 x 4 tile's 32, and fits the problem exactly:
//   phase 1   S[r][k] = sum_t V[t][r] x[c_t][k]    block b = fragments 4 b + (0..3), i = fragment, j = draw (k = 4 kg + j,
//             kg < ceil(K / 4)): one instruction per transcript t and draw group, A = V[t][lane] -- one 4-byte LDS read
//             per lane and transcript -- and B = x[c_t][4 kg + (lane & 3)], constant over a run (registers);
//             d1[kg], register i of lane (b, j) = S[4 b + i][4 kg + j]
//   weights   W = ks / S in place (v_rcp_f32): 4 ceil(K / 4) reciprocals per lane instead of 16
//   phase 2   G[t][k] += sum_r V[t][r] W[r][k]     per group g of 4 transcripts and fragment index i: block b adds the
//             outer product of V[4 g + (0..3)][4 b + i] with W[4 b + i][4 kg + (0..3)] -- B is d1[kg][i] as it stands,
//             A is a 4-byte LDS read of row 4 g + (lane & 3) -- into acc[g][kg]; the sixteen blocks hold partial sums
//             over their four fragments, added across lanes (DPP) when the run is flushed.
// MFMA issue cycles of a slice of w transcripts at K = 6:  64 ceil(w / 4) + 64 ceil(w / 4)  against  128 ceil(w / 4) +
// 256 or 512 before.  Element r of row t is stored at position r ^ (t & 3) of the row (psell_row_pos, stream 0): both
// read patterns -- lane l reads position l ^ (t & 3) of row t; lane (b, i') reads position (4 b + i) ^ i' of row
// 4 g + i' -- then touch 64 different banks.
//
// The loop is written for a short instruction stream (a wave issues at most one instruction every four cycles, and the
// bookkeeping around the matrix instructions was three quarters of what it issued):
//   * the slice body exists in 4 x 2 straight-line versions: groups of four transcripts (1..4) x "the slice's bytes are
//     contiguous in the ring" (every operand address is one per-slice base register plus an immediate offset) or "they
//     wrap around its end" (a third of the slices: addresses computed row by row);
//   * at a run's start lanes t < 16 compute, once, the LDS addresses of transcript t's x row and gradient row (rows
//     t >= w of the last group point at a row of zeros / at a scratch row: no masks in the loads and in the flush);
//   * the flush adds a group's four transcripts under one exec mask.
// `aux_lds`: LDS address of 32 bytes of zeros followed by 32 bytes of scratch.
// 4 x 4 transpose inside every quad of lanes: lane j of a quad ends up with register j of the quad's lanes 0..3 in
// a0..a3 (out[i] of lane j = in[j] of lane i).  Two rounds of "keep or take the neighbour's" with DPP quad permutes
// folded into the selects (v_cndmask_b32_dpp: D = vcc ? src1 : permuted src0) -- 8 vector instructions for 16 values.
// (Inline assembly: the compiler's hazard recogniser does not look inside, so the block starts with the two wait states a
// DPP read of a freshly written VGPR needs; inside it every such pair is at least two instructions apart.)
__device__ inline void quad_transpose(float &a0, float &a1, float &a2, float &a3)
{
    float y0, y1, y2, y3;
    const uint64_t E = 0x5555555555555555ull, L = 0x3333333333333333ull;  // lanes with bit 0 / bit 1 of their index clear
    asm volatile("s_nop 1\n\t"
                 "s_mov_b64 vcc, %8\n\t"
                 "v_cndmask_b32_dpp %4, %1, %0, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"  // y0 = even ? a0 : a1 of lane ^ 1
                 "v_cndmask_b32_dpp %6, %3, %2, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"  // y2 = even ? a2 : a3 of lane ^ 1
                 "s_not_b64 vcc, vcc\n\t"
                 "v_cndmask_b32_dpp %5, %0, %1, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"  // y1 = odd ? a1 : a0 of lane ^ 1
                 "v_cndmask_b32_dpp %7, %2, %3, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"  // y3 = odd ? a3 : a2 of lane ^ 1
                 "s_mov_b64 vcc, %9\n\t"
                 "v_cndmask_b32_dpp %0, %6, %4, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"  // z0 = low ? y0 : y2 of lane ^ 2
                 "v_cndmask_b32_dpp %1, %7, %5, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"  // z1 = low ? y1 : y3 of lane ^ 2
                 "s_not_b64 vcc, vcc\n\t"
                 "v_cndmask_b32_dpp %2, %4, %6, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"  // z2 = high ? y2 : y0 of lane ^ 2
                 "v_cndmask_b32_dpp %3, %5, %7, vcc quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf"        // z3 = high ? y3 : y1 of lane ^ 2
                 : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "=&v"(y0), "=&v"(y1), "=&v"(y2), "=&v"(y3)
                 : "s"(E), "s"(L)
                 : "vcc", "scc");
}

// ---- building blocks of the batched 4 x 4 outer products: narrow_stream (dense and MASKED) and wide_masked_stream ----------
// Lane (b = lane >> 2, j = lane & 3), j4 = 4 j; KG = ceil(K / 4) draw groups; acc[kg], register v of lane (b, j): block b's part
// of G[4 g + v][4 kg + j] for one group g of four transcripts.

// (WANT_LP) per draw group: the log of the product of this lane's row sums (LogAcc above); with multiplicities: the sum of ks log2 s
template <int KG>
struct QuadLp {
    LogAcc lpl[KG];
    double lp2[KG];
    __device__ inline QuadLp()
    {
#pragma unroll
        for (int kg = 0; kg < KG; ++kg) {
            lpl[kg].init();
            lp2[kg] = 0.0;
        }
    }
};

// Flush of a group of four transcripts.  The
// four registers v are first added across the wave's four rows of 16 lanes and scattered (gfx950 lane swaps: row r
// is left with transcript VROW[r]'s sums, block by block), then across a row's four blocks (DPP): lanes 12..15 of
// every row hold one finished sum each and ONE LDS add per (group, draw group) writes 16 different addresses.
// (Adding the rows' partial sums to the same addresses instead -- four-way conflicts in four times as many LDS
// atomics -- cost a quarter of the kernel's time.)
// `ga`: in lanes 12 + j of every row of 16 lanes, the LDS address of draw j of the gradient row of the transcript that row is
// left with.
template <int K>
__device__ inline void quad_flush_sums(f32x4 (&acc)[(K + 3) / 4], uint32_t ga, int lane, int j, int dbg)
{
#pragma unroll
    for (int kg = 0; kg < (K + 3) / 4; ++kg) {
        auto r1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[kg][0]), __float_as_uint(acc[kg][1]), false, false);
        const float ab = __uint_as_float(r1[0]) + __uint_as_float(r1[1]);
        auto r2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[kg][2]), __float_as_uint(acc[kg][3]), false, false);
        const float cd = __uint_as_float(r2[0]) + __uint_as_float(r2[1]);
        auto r3 = __builtin_amdgcn_permlane16_swap(__float_as_uint(ab), __float_as_uint(cd), false, false);
        float q = __uint_as_float(r3[0]) + __uint_as_float(r3[1]);
        q += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(q), 0x114, 0xf, 0xf, true));  // row_shr:4
        q += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(q), 0x118, 0xf, 0xf, true));  // row_shr:8
        if ((lane & 12) == 12 && 4 * kg + j < K && !(dbg & 2))
            __hip_atomic_fetch_add(reinterpret_cast<lds_fp>((uintptr_t)(ga + 16u * (uint32_t)kg)), q, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
        acc[kg] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}
// The rows' transcripts: row 0: transcript 4 g, row 1: 4 g + 2, row 2: 4 g + 1, row 3: 4 g + 3.
// The flush of a loop that flushes every slice (wide_masked_stream): lane t < 16 of `gav` holds the LDS address of transcript
// t's gradient row; group g's addresses by lane reads and selects.
template <int K>
__device__ inline void quad_flush_group(f32x4 (&acc)[(K + 3) / 4], uint32_t gav, int g, int lane, int j, uint32_t j4, int dbg)
{
    const uint32_t ga0 = (uint32_t)__builtin_amdgcn_readlane((int)gav, 4 * g + 0), ga2 = (uint32_t)__builtin_amdgcn_readlane((int)gav, 4 * g + 2);
    const uint32_t ga1 = (uint32_t)__builtin_amdgcn_readlane((int)gav, 4 * g + 1), ga3 = (uint32_t)__builtin_amdgcn_readlane((int)gav, 4 * g + 3);
    const uint32_t ga = ((lane & 32) ? ((lane & 16) ? ga3 : ga1) : ((lane & 16) ? ga2 : ga0)) + j4;
    quad_flush_sums<K>(acc, ga, lane, j, dbg);
}
// The flush of a loop that keeps its sums for a run of slices (narrow_stream): the addresses are a property of the run, so its
// start spreads them ONCE -- `gal`: every row of 16 lanes holds transcript t's address in lane t; result: lane (row r, quad q,
// j) holds draw j of transcript 4 q + (0, 2, 1, 3)[r], i.e. group q's address for this row -- by four quad broadcasts under row
// masks, and the flush of group g moves quad g to the row's last quad with one DPP row shift (none for g = 3) instead of four
// lane reads, four moves and three selects per group and flush.
__device__ inline uint32_t quad_spread_rows(uint32_t gal, uint32_t j4)
{
    const int v = (int)gal;
    int o = __builtin_amdgcn_update_dpp(0, v, 0x00, 0xf, 0xf, true);  // quad_perm:[0,0,0,0], every row
    o = __builtin_amdgcn_update_dpp(o, v, 0xaa, 0x2, 0xf, false);     // quad_perm:[2,2,2,2], row 1
    o = __builtin_amdgcn_update_dpp(o, v, 0x55, 0x4, 0xf, false);     // quad_perm:[1,1,1,1], row 2
    o = __builtin_amdgcn_update_dpp(o, v, 0xff, 0x8, 0xf, false);     // quad_perm:[3,3,3,3], row 3
    return (uint32_t)o + j4;
}
template <int K, int G>
__device__ inline void quad_flush_spread(f32x4 (&acc)[(K + 3) / 4], uint32_t gaq, int lane, int j, int dbg)
{
    // lanes 12 + j of a row read lanes 4 G + j of it (the other lanes' values are not used)
    const uint32_t ga = G == 3 ? gaq : (uint32_t)__builtin_amdgcn_update_dpp(0, (int)gaq, 0x110 + (12 - 4 * G), 0xf, 0xf, true);  // row_shr:12 - 4 G
    quad_flush_sums<K>(acc, ga, lane, j, dbg);
}
// x[c_t][4 kg + j] of transcripts 4 g .. 4 g + 3 (lane t < 16 of `xav`: the LDS address of transcript t's x row)
template <int KG>
__device__ inline void quad_load_x_group(uint32_t xav, int g, uint32_t j4, float (*dst)[KG])
{
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)xav, 4 * g + u) + j4;
        dst[u][0] = lds_f(a);
        if (KG > 1) dst[u][KG > 1 ? 1 : 0] = lds_f(a + 16u);  // (draws >= K: a neighbour's values, in columns that are never used)
    }
}
// the first group of a slice: the chains start from `c0` (the row sums' floor), which stays in its registers
template <int KG>
__device__ inline void quad_phase1_first(f32x4 (&d1)[KG], const f32x4 &c0, const float *p4, const float (*x4)[KG])
{
#pragma unroll
    for (int kg = 0; kg < KG; ++kg) d1[kg] = __builtin_amdgcn_mfma_f32_4x4x1f32(p4[0], x4[0][kg], c0, 0, 0, 0);
#pragma unroll
    for (int u = 1; u < 4; ++u)
#pragma unroll
        for (int kg = 0; kg < KG; ++kg) d1[kg] = __builtin_amdgcn_mfma_f32_4x4x1f32(p4[u], x4[u][kg], d1[kg], 0, 0, 0);
}
template <int KG>
__device__ inline void quad_phase1(f32x4 (&d1)[KG], const float *p4, const float (*x4)[KG])
{
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int kg = 0; kg < KG; ++kg) d1[kg] = __builtin_amdgcn_mfma_f32_4x4x1f32(p4[u], x4[u][kg], d1[kg], 0, 0, 0);
}
// weights, in place: d1[kg][i] of lane (b, j) belongs to fragment 4 b + i, draw 4 kg + j; kv: the fragments' multiplicities
template <int K, bool WANT_LP, bool HAS_KS>
__device__ inline void quad_weights(f32x4 (&d1)[(K + 3) / 4], const f32x4 &kv, int j, QuadLp<(K + 3) / 4> &lp)
{
#pragma unroll
    for (int kg = 0; kg < (K + 3) / 4; ++kg)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float sv = d1[kg][i];
            if (WANT_LP) {
                const bool valid = 4 * kg + j < K && sv > 2.0f * ROWSUM_FLOOR;
                if (HAS_KS) {
                    if (valid) lp.lp2[kg] += ks_log2(kv[i], sv);
                } else {
                    lp.lpl[kg].mul(sv, valid);
                }
            }
            d1[kg][i] = HAS_KS ? kv[i] * __builtin_amdgcn_rcpf(sv) : __builtin_amdgcn_rcpf(sv);  // (padded fragments: ks = 0)
        }
}
template <int KG>
__device__ inline void quad_phase2(f32x4 (&acc)[KG], const f32x4 (&d1)[KG], const float *q4)
{
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int kg = 0; kg < KG; ++kg) acc[kg] = __builtin_amdgcn_mfma_f32_4x4x1f32(q4[i], d1[kg][i], acc[kg], 0, 0, 0);
}
// into the caller's accumulator, whose lane l < 16 collects draw l: the sixteen blocks' sums of draw 4 kg + j
template <int K, bool HAS_KS>
__device__ inline void quad_lp_reduce(const QuadLp<(K + 3) / 4> &lp, int lane, double &lpacc)
{
#pragma unroll
    for (int kg = 0; kg < (K + 3) / 4; ++kg) {
        double v = HAS_KS ? lp.lp2[kg] * 0.693147180559945309417 : lp.lpl[kg].log_value();
        v += __shfl_xor(v, 4, 64);
        v += __shfl_xor(v, 8, 64);
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (lane < 16 && (lane >> 2) == kg && lane < K) lpacc += v;
    }
}

// MASKED: the tile's slices are masked slices (stream A1M, loglik_internal.hpp): a fragment's values are stored packed
// (its i-th non-zero in row i) with a 16-bit mask of the union's transcripts it has.  Lane r expands its own fragment
// for phase 1 -- V[t][r] = bit t of its mask ? row (number of lower mask bits) : 0, one LDS read at a running address per
// transcript, conflict free because every lane reads its own column -- and phase 2's operands V[4 g + j][4 b + i] are
// exactly the quad transposes of the phase-1 registers: no second LDS pass, and the slice's ring bytes are free before
// the first matrix instruction.
template <int K, uint32_t RB, bool WANT_LP, bool HAS_KS, bool MASKED>
__device__ inline void narrow_stream(WaveStream &ws, const char *ring, int extras, const float *xw, float *gw,
                                     uint32_t aux_lds, double &lpacc, int dbg, Stamps &st)
{
    constexpr int WMAX = PSELL_NARROW_MAX;
    static_assert(WMAX == 16, "four groups of four transcripts");
    constexpr int KG = (K + 3) / 4;
    const int lane = wave_lane();  // (see wide_stream: per-tile lane constants instead of spilled ones)
    const uint32_t ring_lds = lds_addr(ring);
    const uint32_t xw_lds = lds_addr(xw), gw_lds = lds_addr(gw);
    const int j = lane & 3, b = lane >> 2;
    const uint32_t j4 = 4u * (uint32_t)j;
    // phase 1 reads position lane ^ (t & 3) of row t; phase 2, fragment index u, position (4 b + u) ^ j = lane ^ u of
    // row 4 g + j: the same four lane constants, plus 256 j
    uint32_t lc1[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) lc1[u] = ring_lds + ((uint32_t)(lane ^ u) << 2);
    const uint32_t j256 = 256u * (uint32_t)j;

    f32x4 acc[4][KG];  // acc[g][kg], register v of lane (b, j): block b's part of G[4 g + v][4 kg + j]
    float xq[8][KG];   // x[c_t][4 kg + j] of the run's first eight transcripts (the others': re-read per slice, see below)
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int kg = 0; kg < KG; ++kg) acc[g][kg] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int kg = 0; kg < KG; ++kg) xq[t][kg] = 0.0f;
    uint32_t xav = aux_lds;         // lane t < 16: LDS address of the x row of the run's transcript t
    uint32_t gaq = aux_lds + 32u;  // the gradient rows' addresses, spread for the flush (quad_spread_rows)
    int pend_w = 0;
    int run_w = 0;  // (MASKED) transcripts of the current run's union
    QuadLp<KG> lp;  // (WANT_LP)
    // the row sums' start value, as the C operand of each chain's first matrix instruction: four registers held across the loop
    // instead of moves into every chain's accumulator in every slice (the addend and the order of the sums are the same)
    f32x4 floorq = f32x4{ROWSUM_FLOOR, ROWSUM_FLOOR, ROWSUM_FLOOR, ROWSUM_FLOOR};
    asm volatile("" : "+v"(floorq));  // (opaque: not rematerialised per slice)

    auto flush = [&]() {
        quad_flush_spread<K, 0>(acc[0], gaq, lane, j, dbg);
        if (pend_w > 4) quad_flush_spread<K, 1>(acc[1], gaq, lane, j, dbg);
        if (pend_w > 8) quad_flush_spread<K, 2>(acc[2], gaq, lane, j, dbg);
        if (pend_w > 12) quad_flush_spread<K, 3>(acc[3], gaq, lane, j, dbg);
        pend_w = 0;
    };

    RingCursor<RB, true> rc(ws, ring_lds, extras, lc1[0]);  // (the tail stands at the current slice; lc1[0] = ring_lds + 4 x lane)
    uint32_t e_next = (uint32_t)__builtin_amdgcn_readlane((int)ws.ent, 0);  // (a slice's end is the next one's start: one lane read per slice)
    for (int si = 0; si < ws.nsl; ++si) {
        const uint32_t e0 = e_next;
        const uint32_t e1 = (uint32_t)__builtin_amdgcn_readlane((int)ws.ent, si + 1);
        e_next = e1;
        const SliceEntry se = slice_entry(e0, e1);
        const int flags = se.flags;
        const int nrows = (int)(se.units / 2u) - 1 - (HAS_KS ? 1 : 0);  // rows of 64 values: the set's transcripts / (MASKED) the longest fragment
        int w = MASKED ? run_w : nrows;
        const uint32_t bytes = se.bytes;
        if (!(dbg & 16)) __builtin_amdgcn_s_setprio(3);
        STAMP(1);  // slice bookkeeping
        rc.wait_for_steady(bytes);
        STAMP(2);  // waiting for the DMA
        if (pend_w != 0 && !(flags & 2)) flush();
        if (pend_w == 0 && !((dbg & 64) && si > 0)) {
            // a new run: lane t < 16 reads transcript t's tile-local id from the slice's header and turns it into the
            // addresses of its x row and its gradient row; then the x values of the run, four transcripts at a time
            const uint32_t cid = *reinterpret_cast<lds_cu16p>(
                (uintptr_t)(ring_lds + rc.pos_r + (MASKED ? 4u * (uint32_t)(lane & 15) + 2u : 2u * (uint32_t)(lane & 15))));
            const bool live = MASKED ? cid != (uint32_t)PSELL_NO_COL : (lane & 15) < w;
            if (MASKED) {
                run_w = __builtin_popcount((uint32_t)__ballot(live) & 0xffffu);
                w = run_w;
            }
            xav = live ? xw_lds + cid * (uint32_t)(K * 4) : aux_lds;
            gaq = quad_spread_rows(live ? gw_lds + cid * (uint32_t)(K * 4) : aux_lds + 32u, j4);
            quad_load_x_group(xav, 0, j4, xq);
            if (w > 4) quad_load_x_group(xav, 1, j4, xq + 4);
        }
        STAMP(3);  // run change: flush + column lookup

        const uint32_t row0 = wrap_u<RB>(rc.pos_r + 256u);
        f32x4 d1[KG];  // (every chain starts from floorq: quad_phase1_first)
        f32x4 kv = f32x4{1.f, 1.f, 1.f, 1.f};
        // NG = groups of four transcripts of the slice; FAST = its bytes do not wrap around the ring's end
        auto body = [&](auto NGc, auto FASTc) {
            constexpr int NG = decltype(NGc)::value;
            constexpr bool FAST = decltype(FASTc)::value;
            float pv[8], qv[2][4];  // the operands of two groups at a time
            uint32_t bp[4];
            if (FAST) {
#pragma unroll
                for (int u = 0; u < 4; ++u) bp[u] = lc1[u] + rc.pos_r;
            }
            auto read_p = [&](int g0, int g1) {  // phase-1 operands of groups g0 .. g1 - 1: V[t][lane]
#pragma unroll
                for (int g = g0; g < g1; ++g) {
                    if (FAST) {
#pragma unroll
                        for (int u = 0; u < 4; ++u) pv[4 * (g - g0) + u] = lds_f(bp[u] + 256u + 1024u * (uint32_t)g + 256u * (uint32_t)u);
                    } else {
                        const uint32_t rg = wrap_u<RB>(row0 + 1024u * (uint32_t)g);  // row 4 g
#pragma unroll
                        for (int u = 0; u < 4; ++u) pv[4 * (g - g0) + u] = lds_f(lc1[u] + wrap_u<RB>(rg + 256u * (uint32_t)u));
                    }
                }
            };
            auto read_q = [&](int g0, int g1) {  // phase-2 operands: V[4 g + j][4 b + u]
#pragma unroll
                for (int g = g0; g < g1; ++g) {
                    if (FAST) {
#pragma unroll
                        for (int u = 0; u < 4; ++u) qv[g - g0][u] = lds_f(bp[u] + j256 + 256u + 1024u * (uint32_t)g);
                    } else {
                        const uint32_t rg = wrap_u<RB>(row0 + 1024u * (uint32_t)g);
                        const uint32_t jr = rg + 256u * (uint32_t)j;
                        const uint32_t back = jr >= RB ? RB : 0u;  // (the ring's end may fall inside this group of rows)
#pragma unroll
                        for (int u = 0; u < 4; ++u) qv[g - g0][u] = lds_f(lc1[u] + j256 + rg - back);
                    }
                }
            };
            if (HAS_KS)  // the multiplicities travel with the slice (its last row, stored in fragment order)
                kv = *reinterpret_cast<const f32x4 *>(ring + wrap_u<RB>(row0 + 256u * (uint32_t)nrows) + 16u * (uint32_t)b);
            if (MASKED) {
                // this lane's fragment, expanded by its mask: transcript t of the union is in row (number of mask bits
                // below t) of the slice when bit t is set; `a` runs through the rows' addresses.  Rows past the fragment's
                // last non-zero (and past the slice: the bytes behind it in the ring) are read and masked away.
                const uint32_t mk = *reinterpret_cast<lds_cu16p>(
                    (uintptr_t)(lc1[0] + rc.pos_r));  // low half of header word `lane`
                float mv[4 * NG];
                uint32_t a = lc1[0] + row0;
                const uint32_t lim = lc1[0] + RB;  // (slices that wrap around the ring's end)
#pragma unroll
                for (int t = 0; t < 4 * NG; ++t) {
                    mv[t] = lds_f(a);
                    a += ((mk >> t) & 1u) << 8;
                    if (!FAST) a = a >= lim ? a - RB : a;
                }
                slice_consumed([&] { rc.advance(bytes); }, st, dbg);
#pragma unroll
                for (int t = 0; t < 4 * NG; ++t) mv[t] = __uint_as_float(__float_as_uint(mv[t]) & (uint32_t)(((int)(mk << (31 - t))) >> 31));
                quad_phase1_first(d1, floorq, mv, xq);
                if (NG > 1) quad_phase1(d1, mv + 4, xq + 4);
                if (NG > 2) {  // (registers hold the x rows of eight transcripts: the others' are re-read per slice)
                    float xr[8][KG];
                    quad_load_x_group(xav, 2, j4, xr);
                    if (NG > 3) quad_load_x_group(xav, 3, j4, xr + 4);
                    quad_phase1(d1, mv + 8, xr);
                    if (NG > 3) quad_phase1(d1, mv + (NG > 3 ? 12 : 0), xr + 4);
                }
                quad_weights<K, WANT_LP, HAS_KS>(d1, kv, j, lp);
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    quad_transpose(mv[4 * g], mv[4 * g + 1], mv[4 * g + 2], mv[4 * g + 3]);
                    quad_phase2(acc[g], d1, mv + 4 * g);
                }
            } else if (NG <= 2) {
                // all operands at once; the slice's ring bytes are free before the matrix phases
                read_p(0, NG);
                read_q(0, NG);
                slice_consumed([&] { rc.advance(bytes); }, st, dbg);
                quad_phase1_first(d1, floorq, pv, xq);
                if (NG > 1) quad_phase1(d1, pv + 4, xq + 4);
                quad_weights<K, WANT_LP, HAS_KS>(d1, kv, j, lp);
                quad_phase2(acc[0], d1, qv[0]);
                if (NG > 1) quad_phase2(acc[1], d1, qv[1]);
            } else {
                // (registers hold the x rows of eight transcripts: those of the third and fourth group are re-read from
                // the window for every slice.)  Two LDS round trips: the phase-1 operands, then -- overlapping the
                // reciprocals -- the phase-2 operands, in the registers the first ones have left
                float pw[8], xr[8][KG], qw[2][4];
                read_p(0, 2);
#pragma unroll
                for (int u = 0; u < 8; ++u) pw[u] = pv[u];
                read_p(2, NG);
                if (!(dbg & 4)) {
                    quad_load_x_group(xav, 2, j4, xr);
                    if (NG > 3) quad_load_x_group(xav, 3, j4, xr + 4);
                } else {
#pragma unroll
                    for (int u = 0; u < 8; ++u)
#pragma unroll
                        for (int kg = 0; kg < KG; ++kg) xr[u][kg] = xq[u][kg];
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (!(dbg & 16)) __builtin_amdgcn_s_setprio(0);
                quad_phase1_first(d1, floorq, pw, xq);
                quad_phase1(d1, pw + 4, xq + 4);
                quad_phase1(d1, pv, xr);
                if (NG > 3) quad_phase1(d1, pv + 4, xr + 4);
                read_q(0, 2);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    qw[0][u] = qv[0][u];
                    qw[1][u] = qv[1][u];
                }
                read_q(2, NG);
                quad_weights<K, WANT_LP, HAS_KS>(d1, kv, j, lp);
                slice_consumed([&] { rc.advance(bytes); }, st, dbg);
                quad_phase2(acc[0], d1, qw[0]);
                quad_phase2(acc[1], d1, qw[1]);
                quad_phase2(acc[2], d1, qv[0]);
                if (NG > 3) quad_phase2(acc[3], d1, qv[1]);
            }
        };
        // (The ladder stays written out here and in wide_masked_stream.  As a shared helper that takes `body` it changed the order
        // in which the eight bodies are inlined: other scalar code in this loop, and the pass 0.6 % slower on long runs of
        // narrow dense slices, profiles/stream_refactor_bench.txt.)
        {
            using std::integral_constant;
            const bool fast = rc.pos_r + bytes <= RB;
            if (fast) {
                if (w <= 4) body(integral_constant<int, 1>(), integral_constant<bool, true>());
                else if (w <= 8) body(integral_constant<int, 2>(), integral_constant<bool, true>());
                else if (w <= 12) body(integral_constant<int, 3>(), integral_constant<bool, true>());
                else body(integral_constant<int, 4>(), integral_constant<bool, true>());
            } else {
                if (w <= 4) body(integral_constant<int, 1>(), integral_constant<bool, false>());
                else if (w <= 8) body(integral_constant<int, 2>(), integral_constant<bool, false>());
                else if (w <= 12) body(integral_constant<int, 3>(), integral_constant<bool, false>());
                else body(integral_constant<int, 4>(), integral_constant<bool, false>());
            }
        }
        pend_w = w;
        STAMP(5);  // phase 2
    }
    if (pend_w != 0) flush();
    if (WANT_LP) quad_lp_reduce<K, HAS_KS>(lp, lane, lpacc);
}

// ---- the slice loop of the MIXED NARROW stream (BN: unrelated fragments of <= 16 transcripts) ----------------------------
// Lane = fragment, any 64 fragments of the tile: val[w][64]; lcol[w][64] (tile-local ids, 16 bit).  Two sweeps over the
// slice in the wave's LDS ring: row sums by gathers from the tile's x window, then the gradient contributions summed per
// run of lanes with the same transcript (segmented DPP scan) and added to the tile's gradient window by the last lane of
// every run.  ~3x the instructions of a matrix-core slice per entry, but 64 fragments per slice whatever their sets: the
// place for fragments without company, inside the same launch.  Every LDS access names its address space: a generic
// (flat) access would count against vmcnt and break the ring's counted waits.
template <int K>
__device__ inline void scatter_runs_lds(int c, float (&q)[K], uint32_t gw_lds, int lane)
{
    auto add = [](uint32_t a, float v) {
        __hip_atomic_fetch_add(reinterpret_cast<lds_fp>((uintptr_t)a), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    const int c0 = __builtin_amdgcn_readfirstlane(c);
    if (__all(c == c0)) {  // one column for the whole wavefront: plain wave sum
        wave_sum_to_lane63_n<K>(q);
        if (lane == 63) {
#pragma unroll
            for (int k = 0; k < K; ++k) add(gw_lds + (uint32_t)(c0 * K + k) * 4u, q[k]);
        }
        return;
    }
    const int cprev = __builtin_amdgcn_update_dpp(-1, c, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
    const unsigned long long heads = __ballot(c != cprev);  // lane 0 compares with -1: always a head
    const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
    const int dist = lane - (63 - __clzll(heads & upto));  // distance to the head of this lane's run
    const int rl = lane & 15;
    const float m1 = dist >= 1 ? 1.f : 0.f, m2 = dist >= 2 ? 1.f : 0.f, m4 = dist >= 4 ? 1.f : 0.f,
                m8 = dist >= 8 ? 1.f : 0.f;
    const float mb15 = dist > rl ? 1.f : 0.f;           // run started in an earlier row of 16
    const float mb31 = dist > (lane & 31) ? 1.f : 0.f;  // run started before lane 32
#pragma unroll
    for (int k = 0; k < K; ++k) q[k] = fmaf(dpp_mov0<0x111, 0xf>(q[k]), m1, q[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) q[k] = fmaf(dpp_mov0<0x112, 0xf>(q[k]), m2, q[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) q[k] = fmaf(dpp_mov0<0x114, 0xf>(q[k]), m4, q[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) q[k] = fmaf(dpp_mov0<0x118, 0xf>(q[k]), m8, q[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) q[k] = fmaf(dpp_mov0<0x142, 0xa>(q[k]), mb15, q[k]);  // row_bcast:15 -> rows 1, 3
#pragma unroll
    for (int k = 0; k < K; ++k) q[k] = fmaf(dpp_mov0<0x143, 0xc>(q[k]), mb31, q[k]);  // row_bcast:31 -> rows 2, 3
    const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
    if (tail) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (q[k] != 0.0f) add(gw_lds + (uint32_t)(c * K + k) * 4u, q[k]);
    }
}

template <int K, uint32_t RB, bool WANT_LP, bool HAS_KS>
__device__ inline void mixed_stream(WaveStream &ws, const char *ring, int extras, const float *xw, float *gw, double &lpacc, int dbg, Stamps &st)
{
    const int lane = wave_lane();
    const uint32_t ring_lds = lds_addr(ring);
    const uint32_t xw_lds = lds_addr(xw), gw_lds = lds_addr(gw);
    const uint32_t la4 = ring_lds + 4u * (uint32_t)lane, la2 = ring_lds + 2u * (uint32_t)lane;
    auto x_row_fma = [&](float v, uint32_t c, float (&sacc)[K]) {  // sacc[k] += v x[c][k]
        const uint32_t a = xw_lds + c * (uint32_t)(K * 4);
        if constexpr (K % 2 == 0) {
#pragma unroll
            for (int k = 0; k < K / 2; ++k) {
                const f32x2 x = *reinterpret_cast<lds_cf2p>((uintptr_t)(a + 8u * (uint32_t)k));
                sacc[2 * k] = fmaf(v, x.x, sacc[2 * k]);
                sacc[2 * k + 1] = fmaf(v, x.y, sacc[2 * k + 1]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k) sacc[k] = fmaf(v, *reinterpret_cast<lds_cfp>((uintptr_t)(a + 4u * (uint32_t)k)), sacc[k]);
        }
    };
    LogAcc lpl[WANT_LP ? K : 1];  // (WANT_LP) per draw (LogAcc above); with multiplicities lp2 = sum ks log2 s
    double lp2[WANT_LP ? K : 1];
#pragma unroll
    for (int k = 0; k < (WANT_LP ? K : 1); ++k) {
        lpl[k].init();
        lp2[k] = 0.0;
    }

    uint32_t pos = 0, pos_r = 0;
    for (int si = 0; si < ws.nsl; ++si) {
        const uint32_t e0 = (uint32_t)__builtin_amdgcn_readlane((int)ws.ent, si);
        const uint32_t e1 = (uint32_t)__builtin_amdgcn_readlane((int)ws.ent, si + 1);
        const uint32_t units = slice_entry(e0, e1).units;
        const int w = (int)((units - (HAS_KS ? 2u : 0u)) / 3u);  // float val[w][64]; uint16 lcol[w][64]; padding to 256 B; (float ks[64])
        const uint32_t bytes = units * 128u;
        STAMP(1);
        stream_wait_for<RB>(ws, ring_lds, pos, bytes, extras);
        STAMP(2);
        const uint32_t cols0 = pos_r + 256u * (uint32_t)w;  // (not wrapped yet)
        float sacc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) sacc[k] = 0.0f;
        for (int t = 0; t < w; ++t) {
            const float v = *reinterpret_cast<lds_cfp>((uintptr_t)(la4 + wrap_u<RB>(pos_r + 256u * (uint32_t)t)));
            const uint32_t c = *reinterpret_cast<lds_cu16p>((uintptr_t)(la2 + wrap_u<RB>(cols0 + 128u * (uint32_t)t)));
            x_row_fma(v, c, sacc);
        }
        float ksv = 1.0f;
        if (HAS_KS) ksv = *reinterpret_cast<lds_cfp>((uintptr_t)(la4 + wrap_u<RB>(pos_r + bytes - 256u)));
        float wk[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            wk[k] = fast_weight(ksv, sacc[k]);  // (lanes without a fragment: s = 0, weight 0)
            if (WANT_LP) {
                if (HAS_KS) {
                    if (sacc[k] > 0.0f) lp2[WANT_LP ? k : 0] += ks_log2(ksv, sacc[k]);
                } else {
                    lpl[WANT_LP ? k : 0].mul(sacc[k], sacc[k] > 0.0f);
                }
            }
        }
        STAMP(4);
        for (int t = 0; t < w; ++t) {
            const float v = *reinterpret_cast<lds_cfp>((uintptr_t)(la4 + wrap_u<RB>(pos_r + 256u * (uint32_t)t)));
            const int c = (int)*reinterpret_cast<lds_cu16p>((uintptr_t)(la2 + wrap_u<RB>(cols0 + 128u * (uint32_t)t)));
            float q[K];
#pragma unroll
            for (int k = 0; k < K; ++k) q[k] = v * wk[k];
            if (!(dbg & 2)) scatter_runs_lds<K>(c, q, gw_lds, lane);
        }
        STAMP(5);
        // the slice is consumed: refill the ring behind it
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        stream_advance<RB>(ws, ring_lds, pos, pos_r, bytes);
        STAMP(6);
    }
    if (WANT_LP) {
        // into the caller's accumulator, whose lane l < 16 collects draw l
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double v = HAS_KS ? lp2[WANT_LP ? k : 0] * 0.693147180559945309417 : lpl[WANT_LP ? k : 0].log_value();
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
            if (lane == k) lpacc += v;
        }
    }
}

// ---- the slice loop of the WIDE MASKED stream (A2M: unions of 17..32 transcripts, fragments whose sets differ) ------------
// The narrow masked formulation (lane = fragment, batched 4 x 4 outer products, phase-2 operands by quad transposes) with
// the union's transcripts in two halves: phase 1 runs over all of them, the weights follow, then phase 2 and the flush
// of the first sixteen transcripts' gradients and of the rest -- one set of accumulators serves both halves, so nothing
// stays in registers across slices (leftover fragments rarely come in runs of slices with the same union; when they do,
// only the header work is saved).  Header: two rows of uint32 hw[64]: the low halves are bits 0..15 / 16..31 of the
// fragment's mask, the high halves of the first sixteen words of a row the tile-local ids of transcripts 0..15 / 16..31
// (PSELL_NO_COL past the union) -- every word a finite float, see loglik_internal.hpp.  Two waves of the workgroup work on
// such a tile, with the wide stream's 14 KiB rings (a slice is up to 2 + 32 + 1 rows).
template <int K, uint32_t RB, bool WANT_LP, bool HAS_KS>
__device__ inline void wide_masked_stream(WaveStream &ws, const char *ring, int extras, const float *xw, float *gw,
                                          uint32_t aux_lds, double &lpacc, int dbg, Stamps &st)
{
    constexpr int KG = (K + 3) / 4;
    const int lane = wave_lane();
    const uint32_t ring_lds = lds_addr(ring);
    const uint32_t xw_lds = lds_addr(xw), gw_lds = lds_addr(gw);
    const int j = lane & 3, b = lane >> 2;
    const uint32_t j4 = 4u * (uint32_t)j;
    const uint32_t la = ring_lds + 4u * (uint32_t)lane;  // this lane's column of a row of the ring
    f32x4 acc[4][KG];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int kg = 0; kg < KG; ++kg) acc[g][kg] = f32x4{0.f, 0.f, 0.f, 0.f};
    // lane t < 16: LDS addresses of the x row / gradient row of the union's transcripts t and 16 + t
    uint32_t xav0 = aux_lds, gav0 = aux_lds + 32u, xav1 = aux_lds, gav1 = aux_lds + 32u;
    int run_w = 0;
    QuadLp<KG> lp;  // (WANT_LP)

    uint32_t pos = 0, pos_r = 0;
    for (int si = 0; si < ws.nsl; ++si) {
        const uint32_t e0 = (uint32_t)__builtin_amdgcn_readlane((int)ws.ent, si);
        const uint32_t e1 = (uint32_t)__builtin_amdgcn_readlane((int)ws.ent, si + 1);
        const SliceEntry se = slice_entry(e0, e1);
        const int flags = se.flags;
        const int nrows = (int)(se.units / 2u) - 2 - (HAS_KS ? 1 : 0);  // rows of 64 values = the longest fragment of the slice
        const uint32_t bytes = se.bytes;
        if (!(dbg & 16)) __builtin_amdgcn_s_setprio(3);
        STAMP(1);
        stream_wait_for<RB>(ws, ring_lds, pos, bytes, extras);
        STAMP(2);
        const uint32_t hdr1 = wrap_u<RB>(pos_r + 256u);  // second header row
        if (run_w == 0 || !(flags & 2)) {
            // a new union: lane t < 16 turns the tile-local ids of transcripts t and 16 + t into the addresses of their x
            // rows and gradient rows
            const uint32_t c0 = *reinterpret_cast<lds_cu16p>((uintptr_t)(ring_lds + pos_r + 4u * (uint32_t)(lane & 15) + 2u));
            const uint32_t c1 = *reinterpret_cast<lds_cu16p>((uintptr_t)(ring_lds + hdr1 + 4u * (uint32_t)(lane & 15) + 2u));
            const bool live0 = c0 != (uint32_t)PSELL_NO_COL, live1 = c1 != (uint32_t)PSELL_NO_COL;
            run_w = __builtin_popcount((uint32_t)__ballot(live0) & 0xffffu) + __builtin_popcount((uint32_t)__ballot(live1) & 0xffffu);
            xav0 = live0 ? xw_lds + c0 * (uint32_t)(K * 4) : aux_lds;
            gav0 = live0 ? gw_lds + c0 * (uint32_t)(K * 4) : aux_lds + 32u;
            xav1 = live1 ? xw_lds + c1 * (uint32_t)(K * 4) : aux_lds;
            gav1 = live1 ? gw_lds + c1 * (uint32_t)(K * 4) : aux_lds + 32u;
        }
        STAMP(3);
        const uint32_t mk = (uint32_t)*reinterpret_cast<lds_cu16p>((uintptr_t)(la + pos_r)) |
                            ((uint32_t)*reinterpret_cast<lds_cu16p>((uintptr_t)(la + hdr1)) << 16);
        const uint32_t row0 = wrap_u<RB>(pos_r + 512u);
        f32x4 d1[KG];
#pragma unroll
        for (int kg = 0; kg < KG; ++kg) d1[kg] = f32x4{ROWSUM_FLOOR, ROWSUM_FLOOR, ROWSUM_FLOOR, ROWSUM_FLOOR};
        f32x4 kv = f32x4{1.f, 1.f, 1.f, 1.f};
        auto body = [&](auto NGHc, auto FASTc) {
            constexpr int NGH = decltype(NGHc)::value;  // groups of four transcripts in the second half
            constexpr bool FAST = decltype(FASTc)::value;
            float mvA[16], mvB[4 * NGH];
            uint32_t a = la + row0;
            const uint32_t lim = la + RB;
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                mvA[t] = lds_f(a);
                a += ((mk >> t) & 1u) << 8;
                if (!FAST) a = a >= lim ? a - RB : a;
            }
#pragma unroll
            for (int t = 0; t < 4 * NGH; ++t) {
                mvB[t] = lds_f(a);
                a += ((mk >> (16 + t)) & 1u) << 8;
                if (!FAST) a = a >= lim ? a - RB : a;
            }
            if (HAS_KS) kv = *reinterpret_cast<const f32x4 *>(ring + wrap_u<RB>(row0 + 256u * (uint32_t)nrows) + 16u * (uint32_t)b);
            slice_consumed([&] { stream_advance<RB>(ws, ring_lds, pos, pos_r, bytes); }, st, dbg);
#pragma unroll
            for (int t = 0; t < 16; ++t) mvA[t] = __uint_as_float(__float_as_uint(mvA[t]) & (uint32_t)(((int)(mk << (31 - t))) >> 31));
#pragma unroll
            for (int t = 0; t < 4 * NGH; ++t) mvB[t] = __uint_as_float(__float_as_uint(mvB[t]) & (uint32_t)(((int)(mk << (15 - t))) >> 31));
#pragma unroll
            for (int g = 0; g < 4; g += 2) {
                float xr[8][KG];
                quad_load_x_group(xav0, g, j4, xr);
                quad_load_x_group(xav0, g + 1, j4, xr + 4);
                quad_phase1(d1, mvA + 4 * g, xr);
                quad_phase1(d1, mvA + 4 * g + 4, xr + 4);
            }
#pragma unroll
            for (int g = 0; g < NGH; g += 2) {
                float xr[8][KG];
                quad_load_x_group(xav1, g, j4, xr);
                if (g + 1 < NGH) quad_load_x_group(xav1, g + 1, j4, xr + 4);
                quad_phase1(d1, mvB + 4 * g, xr);
                if (g + 1 < NGH) quad_phase1(d1, mvB + (g + 1 < NGH ? 4 * g + 4 : 0), xr + 4);
            }
            quad_weights<K, WANT_LP, HAS_KS>(d1, kv, j, lp);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                quad_transpose(mvA[4 * g], mvA[4 * g + 1], mvA[4 * g + 2], mvA[4 * g + 3]);
                quad_phase2(acc[g], d1, mvA + 4 * g);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) quad_flush_group<K>(acc[g], gav0, g, lane, j, j4, dbg);
#pragma unroll
            for (int g = 0; g < NGH; ++g) {
                quad_transpose(mvB[4 * g], mvB[4 * g + 1], mvB[4 * g + 2], mvB[4 * g + 3]);
                quad_phase2(acc[g], d1, mvB + 4 * g);
            }
#pragma unroll
            for (int g = 0; g < NGH; ++g) quad_flush_group<K>(acc[g], gav1, g, lane, j, j4, dbg);
        };
        {
            using std::integral_constant;
            const bool fast = pos_r + bytes <= RB;
            const int w = run_w;
            if (fast) {
                if (w <= 20) body(integral_constant<int, 1>(), integral_constant<bool, true>());
                else if (w <= 24) body(integral_constant<int, 2>(), integral_constant<bool, true>());
                else if (w <= 28) body(integral_constant<int, 3>(), integral_constant<bool, true>());
                else body(integral_constant<int, 4>(), integral_constant<bool, true>());
            } else {
                if (w <= 20) body(integral_constant<int, 1>(), integral_constant<bool, false>());
                else if (w <= 24) body(integral_constant<int, 2>(), integral_constant<bool, false>());
                else if (w <= 28) body(integral_constant<int, 3>(), integral_constant<bool, false>());
                else body(integral_constant<int, 4>(), integral_constant<bool, false>());
            }
        }
        STAMP(5);
    }
    if (WANT_LP) quad_lp_reduce<K, HAS_KS>(lp, lane, lpacc);
}

#ifdef POLEE_TILE_CYCLES
extern "C" int polee_debug_read_tile_cycles(unsigned long long *tiles, int ntiles, unsigned long long *wgs, int nwgs)
{
    if (hipMemcpyFromSymbol(tiles, HIP_SYMBOL(g_tile_cycles), sizeof(unsigned long long) * (size_t)ntiles) != hipSuccess) return 1;
    if (hipMemcpyFromSymbol(wgs, HIP_SYMBOL(g_wg_cycles), sizeof(unsigned long long) * (size_t)nwgs) != hipSuccess) return 1;
    static unsigned long long z[1 << 17];
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_tile_cycles), z, sizeof(unsigned long long) * (1 << 17)) != hipSuccess) return 1;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_wg_cycles), z, sizeof(unsigned long long) * 4096) == hipSuccess ? 0 : 1;
}
#endif
#ifdef POLEE_STAMPS
extern "C" int polee_debug_read_stamps(unsigned long long *out)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 24) != hipSuccess) return 1;
    unsigned long long z[24] = {0};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof z) == hipSuccess ? 0 : 1;
}
// the same per wave index: out[4][24]; entry 19 = the wait for the ticket (wave 0)
extern "C" int polee_debug_read_stamps_wave(unsigned long long *out)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps_wave), sizeof(unsigned long long) * 96) != hipSuccess) return 1;
    unsigned long long z[96] = {0};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_stamps_wave), z, sizeof z) == hipSuccess ? 0 : 1;
}
#endif

// LDS layout of the streaming kernel:
//   [rings: 4 x 7 KiB (all kinds but A2M) or 2 x 14 KiB (A2M)][xw 0][xw 1][gw (x 4 in deterministic mode)][ids 0][ids 1][ent 4 x 64][desc 2 x 64][aux 16]
constexpr uint32_t STREAM_RB1 = 7168u, STREAM_RB2 = 14336u, STREAM_RINGS = 28672u;
template <int K>
constexpr uint32_t stream_ring_total()
{
    return STREAM_RINGS;
}
template <int K>
constexpr uint32_t stream_xw_bytes()  // whole 1 KiB pieces
{
    return ((uint32_t)PSELL_TILE_COLS_TARGET * K * 4u + 1023u) & ~1023u;
}
template <int K, bool DET>
constexpr uint32_t stream_lds_bytes()  // (deterministic mode: one gradient window per wave)
{
    return stream_ring_total<K>() + (DET ? 6u : 3u) * stream_xw_bytes<K>() + 2u * PSELL_TILE_COLS_TARGET * 4u + 4u * 256u + 2u * 256u + 64u;
}

// DET: the deterministic mode -- bitwise reproducible gradients: each wave accumulates into its own LDS window (a wave's
// LDS adds retire in program order), the tile's flush sums the four windows in wave order and STORES the result to the
// tile's slot of gwin, and gwin_reduce_kernel adds a transcript's slots in tile order.
template <int K, bool WANT_LP, bool HAS_KS, bool DET>
// (The instances that also return lp carry the log accumulators across the slice loops: at four waves per SIMD -- 128
// registers -- they spill, and a spill's reload drains the LDS-DMA ring (measured: 1.40 ms per pass instead of 0.25).  They run
// three workgroups per CU, 170 registers, no scratch.  Round 5: so do the instances with multiplicities (the factored likelihood of
// salmon's equivalence classes) -- the wide stream's two-stage body holds 32 operand registers across its second stage, and with the
// ks row on top the 128-register instance spilled 11 registers inside the slice loops.)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((WANT_LP || HAS_KS) ? 3 : 4, (WANT_LP || HAS_KS) ? 3 : 4)))
void loglik_stream_kernel(PsellArgs A, int dbg)
{
#ifndef POLEE_ABLATE
    // The ablation switches (POLEE_DBG_ABLATE, tools/probe/time_fit.py) exist only in the diagnostic build `make ablate`: as
    // run-time bits they were live scalar tests in every slice (four branches, four SGPR pairs of masks in a kernel that
    // spills scalar registers); here every `dbg & ...` folds away.
    dbg = 0;
#endif
    extern __shared__ float lds[];
    constexpr uint32_t XWB = stream_xw_bytes<K>();
    constexpr uint32_t GWN = DET ? 4u : 1u;  // gradient windows
    char *const base = reinterpret_cast<char *>(lds);
    char *const rings = base;
    auto xw_of = [&](int b) -> float * { return reinterpret_cast<float *>(base + stream_ring_total<K>() + (uint32_t)b * XWB); };
    float *const gw = reinterpret_cast<float *>(base + stream_ring_total<K>() + 2 * XWB);
    auto ids_of = [&](int b) -> uint32_t * {
        return reinterpret_cast<uint32_t *>(base + stream_ring_total<K>() + (2 + GWN) * XWB + (uint32_t)b * (PSELL_TILE_COLS_TARGET * 4));
    };
    uint32_t *const entb = reinterpret_cast<uint32_t *>(base + stream_ring_total<K>() + (2 + GWN) * XWB + 2 * PSELL_TILE_COLS_TARGET * 4);
    uint32_t *const descb = entb + 4 * 64;  // 2 x 64 words: the schedule entry two rounds ahead, by LDS-DMA
    float *const auxz = reinterpret_cast<float *>(descb + 2 * 64);  // 8 zeros, 8 words of scratch (narrow_stream)

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t G = gridDim.x;
    // Static schedule: every workgroup walks its own column.  Dynamic schedule: one list, longest tile first; a workgroup
    // owns its next two tiles (the next one's x window, ids and offsets are on their way while the current one streams)
    // and wave 0 draws the position after those from a global counter -- one atomic per tile, issued when the tile's slices are
    // done and read at the next tile's start, behind the barriers and the flush.  Workgroups then finish within one (small, late) tile of each other whatever the
    // cost model says: with the static lists the slowest workgroup was 20 - 30 % above the mean (tile times depend on
    // what the neighbours on the CU are doing, not only on the tile).
    const bool dyn = A.dyn_ctr != nullptr;
    const PosDesc *__restrict__ sched = dyn ? A.sched_dyn : A.sched;
    uint32_t p2 = blockIdx.x + 2u * G;  // (wave 0) position of the tile after the next one
    const uint8_t *__restrict__ xwin_b = reinterpret_cast<const uint8_t *>(A.xwin);
    Stamps st;
#ifdef POLEE_STAMPS
    unsigned long long n_slices = 0, n_tiles = 0;
#endif
#ifdef POLEE_TILE_CYCLES
    const unsigned long long t_wg0 = __builtin_amdgcn_s_memtime();
    unsigned long long t_tile0 = t_wg0;
#endif

    // 0 = A1 (dense narrow), 2 = A1M (masked narrow), 1 = A2 (dense wide, in two stages per slice: wide_stream), 4 = BN (mixed
    // narrow): four waves, 7 KiB rings; 3 = A2M (masked wide): two active waves, 14 KiB rings; the schedule holds no others
    auto kind_of = [&](uint32_t tile) -> int { return (int)tile < A.tiles_a1 ? 0 : ((int)tile < A.tiles_a1m ? 2 : ((int)tile < A.tiles_a2 ? 1 : ((int)tile < A.tiles_a ? 3 : 4))); };
    // this wave's share [sb, se) of an A tile's slices: a contiguous block, so that runs stay inside one wave
    auto share = [&](int kind, const PosDesc &t, uint32_t &sb, uint32_t &se) {
        const int nw = kind == 3 ? 2 : 4;
        uint32_t a1 = t.c1, a2 = t.c2, a3 = t.c3;
        asm volatile("" : "+s"(a1), "+s"(a2), "+s"(a3));  // (opaque: or the selects below become an indexed load of a PosDesc kept in scratch memory)
        const uint32_t lo = wave == 0 ? t.s0 : (wave == 1 ? a1 : (wave == 2 ? a2 : a3));
        const uint32_t hi = wave + 1 >= nw ? t.s1 : (wave == 0 ? a1 : (wave == 1 ? a2 : a3));
        sb = wave < nw ? lo : t.s1;
        se = wave < nw ? hi : t.s1;
    };
    // requests everything tile `t` needs besides its slice stream; returns the number of vector-memory operations
    auto prefetch = [&](const PosDesc &t, int buf) -> int {
        int cnt = 0;
        const int npx = (int)((t.L * (uint32_t)K * 4u + 1023u) >> 10);
        const uint8_t *src = xwin_b + (size_t)t.d0 * K * 4;
        const uint32_t dst = lds_addr(xw_of(buf));
        for (int p = wave; p < npx; p += 4) {
            dma_1k_keep(uniform_ptr(src + (size_t)p * 1024), (uint32_t)wave_lane() * 16u, dst + (uint32_t)p * 1024u);
            ++cnt;
        }
        if ((uint32_t)wave * 64u < t.L) {  // transcript ids of the dictionary (for the flush)
            dma_256(uniform_ptr(A.dict + t.d0 + (uint32_t)wave * 64u), min((uint32_t)wave_lane(), t.L - 1u - (uint32_t)wave * 64u) * 4u,
                    lds_addr(ids_of(buf)) + (uint32_t)wave * 256u);
            ++cnt;
        }
        const int kind = kind_of(t.tile);
        {  // slice offsets of this wave's share, one per lane
            uint32_t sb, se;
            share(kind, t, sb, se);
            dma_256(uniform_ptr(A.slice_off + sb), min((uint32_t)wave_lane(), se - sb) * 4u, lds_addr(entb) + (uint32_t)wave * 256u);
            ++cnt;
        }
        return cnt;
    };
    // after the prefetch has landed: this wave's stream state for tile `t`, ring started
    WaveStream ws;
    const int ahead = (dbg >> 8) & 15;  // (experiment: pieces requested ahead; 0 = the whole ring)
    auto start_ring = [&](const PosDesc &t) {
        const int kind = kind_of(t.tile);
        ws.nsl = 0; ws.npieces = 0; ws.issued = 0; ws.slot = 0u; ws.primed = 0; ws.ent = 0u; ws.gsrc = A.data;
        uint32_t sb, se;
        share(kind, t, sb, se);
        ws.ent = entb[wave * 64 + wave_lane()];
        ws.nsl = (int)(se - sb);
        const uint32_t cb = (uint32_t)__builtin_amdgcn_readlane((int)ws.ent, 0) & PSELL_OFF_MASK;
        const uint32_t ce = (uint32_t)__builtin_amdgcn_readlane((int)ws.ent, ws.nsl) & PSELL_OFF_MASK;  // 128-byte units
        ws.npieces = (int)(((ce - cb) * 128u + 1023u) >> 10);
        ws.gsrc = reinterpret_cast<const uint8_t *>(uniform_ptr(A.data + (size_t)cb * 128));
        if (kind != 3) {
            ring_refill<STREAM_RB1>(ws, lds_addr(rings + wave * STREAM_RB1), min(ws.npieces, ahead ? min(ahead, (int)(STREAM_RB1 / 1024u)) : (int)(STREAM_RB1 / 1024u)));
        } else {
            ring_refill<STREAM_RB2>(ws, lds_addr(rings + (wave < 2 ? wave : 0) * STREAM_RB2), min(ws.npieces, ahead ? min(2 * ahead, (int)(STREAM_RB2 / 1024u)) : (int)(STREAM_RB2 / 1024u)));
        }
        ws.primed = ws.issued;
    };

    double lp_a = 0.0;  // lane (tt, q) holds the share of draw tt

    PosDesc cur = sched[blockIdx.x];
    if (cur.tile == POS_NONE) return;  // (the grid never exceeds the number of tiles)
    PosDesc nxt = sched[blockIdx.x + G];
    for (int i = threadIdx.x; i < (int)(GWN * XWB / 4u); i += 256) gw[i] = 0.0f;
    // the rings start out as zeros: operand rows past a slice's last transcript are read (and multiplied by 0), so
    // whatever lies behind a slice in the ring has to be finite
    for (int i = threadIdx.x; i < (int)(stream_ring_total<K>() / 16u); i += 256)
        reinterpret_cast<float4 *>(rings)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (threadIdx.x < 16) auxz[threadIdx.x] = 0.0f;
    lds_barrier();
    (void)prefetch(cur, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    start_ring(cur);
    int young = 0;  // vector-memory operations issued after the ring was started (see wide_stream)
    lds_barrier();
    int buf = 0;
    for (uint32_t round = 0;; ++round) {
        const bool more = nxt.tile != POS_NONE;
        const int kind = kind_of(cur.tile);
        if (more) young += prefetch(nxt, buf ^ 1);
        if (wave == 0) {
            // the schedule entry after the next (a scalar load here would stall every tile by its latency; through LDS it
            // arrives in the background like everything else and is read after the tile's barriers)
            uint32_t off8;  // (lane & 7) * 4, computed here: hoisted out of the tile loop it was spilled, and its reload
                            // (a scratch load the compiler waits for with vmcnt(0)) drained this wave's ring every tile
            asm volatile("v_and_b32_e32 %0, 7, %1\n\tv_lshlrev_b32_e32 %0, 2, %0" : "=v"(off8) : "v"(wave_lane()));
            dma_256(uniform_ptr(sched + p2), off8, lds_addr(descb + (round & 1u) * 64u));
            ++young;
        }
        STAMP(0);  // between tiles: prefetch issue
        // (Round 5 tried WORK STEALING inside the workgroup here -- a wave that had finished its share of the tile's slices stole the
        // tail half of the longest remaining share with an LDS compare-and-swap, the owners taking every slice with an LDS atomic
        // add: correct, and 5 - 12 % SLOWER on every input, profiles/r05_work_stealing_ab.txt.  The static shares stay.)
        {
            const int extras = young;
            if (kind == 0) {
                narrow_stream<K, STREAM_RB1, WANT_LP, HAS_KS, false>(ws, rings + wave * STREAM_RB1, extras, xw_of(buf), gw + (DET ? (uint32_t)wave * (XWB / 4u) : 0u), lds_addr(auxz), lp_a, dbg, st);
            } else if (kind == 2) {
                narrow_stream<K, STREAM_RB1, WANT_LP, HAS_KS, true>(ws, rings + wave * STREAM_RB1, extras, xw_of(buf), gw + (DET ? (uint32_t)wave * (XWB / 4u) : 0u), lds_addr(auxz), lp_a, dbg, st);
            } else if (kind == 4) {
                mixed_stream<K, STREAM_RB1, WANT_LP, HAS_KS>(ws, rings + wave * STREAM_RB1, extras, xw_of(buf), gw + (DET ? (uint32_t)wave * (XWB / 4u) : 0u), lp_a, dbg, st);
            } else if (kind == 3) {
                wide_masked_stream<K, STREAM_RB2, WANT_LP, HAS_KS>(ws, rings + (wave < 2 ? wave : 0) * STREAM_RB2, extras, xw_of(buf), gw + (DET ? (uint32_t)wave * (XWB / 4u) : 0u), lds_addr(auxz), lp_a, dbg, st);
            } else {
                wide_stream<K, STREAM_RB1, WANT_LP, HAS_KS>(ws, rings + wave * STREAM_RB1, extras, xw_of(buf), gw + (DET ? (uint32_t)wave * (XWB / 4u) : 0u), lp_a, dbg, st);
            }
        }
#ifdef POLEE_STAMPS
        n_slices += (unsigned long long)ws.nsl;
        ++n_tiles;
#endif
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (also: the next tile's prefetch has landed)
        STAMP(7);  // draining the queue after the last slice
        young = 0;
        unsigned int drawn = 0u;  // (this tile's draw: defined and consumed inside one iteration, or it is carried -- and spilled -- around the loop)
        if (dyn && wave == 0) {
            // The draw of the position after the next two (one per tile: the host counts on that, dyn_base).  Issued HERE, with the
            // queue empty, and read at the end of this iteration, behind the barriers and the flush: the result occupies a register
            // only in between (until round 5 it was issued at the tile's start and lived across the slice loops).  A compiler-visible
            // atomic: the compiler waits for it with vmcnt(0) where it is read -- by then the next ring's first pieces, requested
            // before the barrier, have had the barrier, the flush and the second barrier to arrive.  (An inline-assembly atomic with a
            // counted wait was tried first: the compiler, unaware that the register is still in flight, copied it -- wrong tickets,
            // tiles skipped; caught by the C2-size oracle tests.)
            if (wave_lane() == 0) drawn = __hip_atomic_fetch_add(A.dyn_ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // a wave that is done starts the next tile's ring BEFORE the barrier when that ring is its own LDS (same kind
        // of uniform tile); otherwise the ring area may still be in use by a slower wave
        const bool early = more && (kind_of(nxt.tile) == 3) == (kind == 3);  // (all kinds but the wide masked one share a ring geometry)
        if (early) start_ring(nxt);
        STAMP(13);  // starting the next ring (before the barrier)
        lds_barrier();  // every wave's contributions are in gw
        STAMP(8);  // waiting for the other waves of the workgroup
        if (more && !early) start_ring(nxt);
        STAMP(13);  // starting the next ring (after the barrier)
        {
            const int LK = (int)cur.L * K;
            const uint32_t *ids = ids_of(buf);
            constexpr int NBF = (PSELL_TILE_COLS_TARGET * K + 255) / 256;
#pragma unroll
            for (int b = 0; b < NBF; ++b) {
                const int i0 = b * 256 + wave * 64;
                if (i0 < LK) {  // (wave-uniform; lane 0 of the wave is active, so the wave issues exactly one atomic here)
                    int i = i0 + wave_lane();
                    asm volatile("" : "+v"(i));  // (keeps i / K from being hoisted out of the tile loop and spilled)
                    if (i < LK) {
                        const int l = i / K;
                        const int k = i - l * K;
                        float v = gw[i];
                        gw[i] = 0.0f;
                        if (DET) {  // the four waves' windows, in wave order; stored to the tile's slot
#pragma unroll
                            for (uint32_t wv = 1; wv < 4; ++wv) {
                                v += gw[wv * (XWB / 4u) + i];
                                gw[wv * (XWB / 4u) + i] = 0.0f;
                            }
                            float *dst = A.gwin + (size_t)cur.d0 * K + i;
                            if (!(dbg & 1)) asm volatile("global_store_dword %0, %1, off" ::"v"(dst), "v"(v) : "memory");
                        } else {
                            float *dst = A.g + (size_t)ids[l] * K + k;
                            if (!(dbg & 1)) asm volatile("global_atomic_add_f32 %0, %1, off" ::"v"(dst), "v"(v) : "memory");
                        }
                    }
                    if (!(dbg & 1)) ++young;  // (younger than the pieces of the ring that has just been started)
                }
            }
        }
        STAMP(15);  // flush issue
        lds_barrier();  // gw is zero again, the next x window is complete
        STAMP(9);  // barrier B
#ifdef POLEE_TILE_CYCLES
        if (threadIdx.x == 0 && cur.tile < (1u << 17)) {
            const unsigned long long now_t = __builtin_amdgcn_s_memtime();
            atomicAdd(&g_tile_cycles[cur.tile], now_t - t_tile0);
            t_tile0 = now_t;
        }
#endif
        if (!more) break;
        cur = nxt;
        if (wave == 0) {
            if (dyn) {
                p2 = min(3u * G + ((uint32_t)__builtin_amdgcn_readfirstlane((int)drawn) - A.dyn_base), A.dyn_last);
            } else {
                p2 += G;
            }
        }
        STAMP(16);  // wave 0: the wait for the ticket (the vmcnt(0) the compiler places in front of the read of `drawn`)
        {
            const uint32_t *dp = descb + (round & 1u) * 64u;
            nxt.tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)dp[0]);
            nxt.s0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)dp[1]);
            nxt.s1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)dp[2]);
            nxt.d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)dp[3]);
            nxt.L = (uint32_t)__builtin_amdgcn_readfirstlane((int)dp[4]);
            nxt.c1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)dp[5]);
            nxt.c2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)dp[6]);
            nxt.c3 = (uint32_t)__builtin_amdgcn_readfirstlane((int)dp[7]);
        }
        buf ^= 1;
    }
    if (WANT_LP && DET) {
        // per-workgroup sums in wave order, stored; gwin_reduce_kernel adds them in workgroup order
        double v = lp_a;
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        double *lpw = reinterpret_cast<double *>(gw);  // (the windows are idle now)
        lds_barrier();
        if (wave_lane() < K) lpw[wave * K + wave_lane()] = v;
        lds_barrier();
        if (threadIdx.x < K) A.lpwin[(size_t)blockIdx.x * K + threadIdx.x] = ((lpw[threadIdx.x] + lpw[K + threadIdx.x]) + lpw[2 * K + threadIdx.x]) + lpw[3 * K + threadIdx.x];
    } else if (WANT_LP) {
        double v = lp_a;
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (wave_lane() < K) atomicAdd(A.lp + wave_lane(), v);
    }
#ifdef POLEE_TILE_CYCLES
    if (threadIdx.x == 0 && blockIdx.x < 4096) atomicAdd(&g_wg_cycles[blockIdx.x], __builtin_amdgcn_s_memtime() - t_wg0);
#endif
#ifdef POLEE_STAMPS
    STAMP(10);
    if (wave_lane() == 0) {
        for (int i = 0; i < 16; ++i) atomicAdd(&g_stamps[i], st.acc[i]);
        atomicAdd(&g_stamps[16], n_slices);
        atomicAdd(&g_stamps[17], n_tiles);
        atomicAdd(&g_stamps[18], 1ull);
        atomicAdd(&g_stamps[19], st.acc[16]);
        unsigned long long *gsw = g_stamps_wave[wave & 3];
        for (int i = 0; i < 16; ++i) atomicAdd(&gsw[i], st.acc[i]);
        atomicAdd(&gsw[16], n_slices);
        atomicAdd(&gsw[17], n_tiles);
        atomicAdd(&gsw[18], 1ull);
        atomicAdd(&gsw[19], st.acc[16]);
    }
#endif
}

}  // namespace polee
