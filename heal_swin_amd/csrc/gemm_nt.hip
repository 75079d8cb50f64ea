// bf16 "NT" GEMM with fused epilogues for the forward and input-gradient products of the path's Linear layers:
//
//     C[m, n] = sum_k A[m, k] * B[n, k]   (+ sum_k A2[m, k] * B2[n, k])   -> epilogue -> bf16
//
// A = activations (token rows, k contiguous), B = a weight as nn.Linear stores it ([out, in], k contiguous); the input
// gradient uses the transposed bf16 weight copy, so it is the same product.  The optional second (A2, B2) segment is the
// decoder's skip connection cat([x, skip]) W^T without the concatenation (swin_hp_transformer.py:772-775).
// Epilogues (fp32 on the accumulators, before the single rounding to bf16):
//     EPI_BIAS   c = acc + bias                                                    (qkv, proj, fc2, reduction, expand, head)
//     EPI_GELU   h = acc + bias -> c ;  aux = dropout(gelu(h))                      (fc1 -> act -> drop, ref :39-41)
//     EPI_DGELU  c = acc * mask * gelu'(aux)                                        (input gradient of fc2 through the GELU)
//     EPI_RESID  c = acc + bias + aux                                               (residual gradient folded into a dgrad)
// so the standalone GELU passes over the 4C-wide hidden tensor (13.5 % of the round-1 step) do not exist.
//
// Structure (gfx950):
//   * workgroup tile BM x BN x 64, waves in WM x WN, each wave (BM/WM) x (BN/WN) as 32x32 accumulators of
//     v_mfma_f32_32x32x16_bf16.  The product is formed TRANSPOSED (D = Bfrag * Afrag^T: accumulator column = m, rows = n),
//     so a lane owns 4 consecutive n of one output row: 8-byte row-major stores, bias as a float4;
//   * operands go global -> LDS by buffer_load ... lds (16 B per lane, 1 KB per wave-instruction), two stages, the loads of
//     step s+1 in flight under the MFMAs of step s; the stream of steps runs ACROSS output tiles (persistent workgroups):
//     the first loads of the next tile are in flight under the epilogue of the current one;
//   * LDS image: tile rows of 128 B paired into 256-B super-rows, 16-byte chunk index XORed with the super-row number
//     (applied to the per-lane SOURCE address of the DMA and to the fragment reads): the 16-lane groups of ds_read_b128
//     touch 16 distinct 16-byte slots (conflict-free), and every 128-B global line is still fetched by 8 adjacent lanes;
//   * tile ids are dealt to XCDs in contiguous ranges (block b runs on XCD b % 8), consecutive ids share the A row panel,
//     so concurrently running workgroups of an XCD re-read A from that XCD's L2;
//   * edges: rows beyond M / N fall outside the buffer descriptors (reads return 0, stores are dropped); a K tail and the
//     n >= N columns are predicated per lane by pointing the access outside the descriptor.
// 128 x 128 tiles run two workgroups per CU (64 KB LDS each): one's epilogue (VALU: erf GELU) overlaps the other's MFMAs.
//
// The file, top to bottom: the optional trace layer; the tile traits (one per variant: everything BM, BN, the wave grid and the
// stage count determine); Operand (the DMA issue side of A or B); the kernel; launch_tile; the shape check and the tile rule
// (pure host functions); the C entry points.
#include <cstdlib>

#include "hs_gelu.h"

namespace hs {
HS_DEFINE_SEED_EPOCH_SETTER(set_seed_epoch_gemm_nt)

// ---- trace layer (measurement build -DHS_GEMM_TRACE, tools/gemm_trace.py): (shader clock << 8 | event code) per wave of workgroups
// 0 and 9, kTraceCap entries each, kept in LDS behind the bias slots and written out when the workgroup ends.  Without the flag
// every piece of it is empty.
#ifdef HS_GEMM_TRACE
#define HS_GEMM_TRACE_PARAM uint64_t* trace;
constexpr int kTraceCap = 240;
static uint64_t* g_trace = nullptr;
extern "C" int hs_gemm_nt_set_trace(void* buf) {
    g_trace = (uint64_t*)buf;
    return 0;
}
template <typename Params>
void trace_attach(Params& p) {
    p.trace = g_trace;
}
// LDS bytes of the event buffers of nw waves behind `used` bytes (the three-stage 256 x 128 tile has no room for them beside the
// bias slots: not traced)
constexpr int trace_lds(int used, int nw) { return used + nw * kTraceCap * 8 <= 163840 ? nw * kTraceCap * 8 : 0; }
struct Trace {
    uint64_t* out;
    bool on;
    int n = 0, nw, wave, lane;
    uint32_t base;
    template <typename Params>
    __device__ __forceinline__ Trace(const Params& p, bool room, uint32_t lds_base, int nw_, int wave_, int lane_)
        : out(p.trace), on(room && p.trace && (blockIdx.x == 0 || blockIdx.x == 9)), nw(nw_), wave(wave_), lane(lane_),
          base(lds_base + wave_ * kTraceCap * 8) {}
    __device__ __forceinline__ void operator()(int code) {
        if (on && n < kTraceCap) {
            const uint64_t t = (clock64() << 8) | (uint64_t)code;
            if (lane == 0) asm volatile("ds_write_b64 %0, %1" ::"v"(base + n * 8), "v"(t) : "memory");
            ++n;
        }
    }
    __device__ __forceinline__ void flush() {
        if (!on) return;
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        uint64_t* dst = out + ((blockIdx.x == 0 ? 0 : 1) * nw + wave) * kTraceCap;
        for (int i = lane; i < kTraceCap; i += 64) {
            uint64_t v = 0;
            if (i < n) {
                asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(base + i * 8) : "memory");
            }
            dst[i] = v;
        }
    }
};
#else
#define HS_GEMM_TRACE_PARAM
template <typename Params>
void trace_attach(Params&) {}
constexpr int trace_lds(int, int) { return 0; }
struct Trace {
    template <typename Params>
    __device__ __forceinline__ Trace(const Params&, bool, uint32_t, int, int, int) {}
    __device__ __forceinline__ void operator()(int) const {}
    __device__ __forceinline__ void flush() const {}
};
#endif

namespace {

typedef unsigned int u32x2 __attribute__((__vector_size__(8)));    // the types the b64 / b128 buffer builtins take
typedef unsigned int u32x4v __attribute__((__vector_size__(16)));

// Cache policy of the epilogue's row-segment stores (gfx950: bit 0 = sc0, bit 1 = nt, bit 4 = sc1).  2 = NON-TEMPORAL:
// an output tile is written once and read by another kernel; stored with the default policy its lines are allocated in the XCD's L2
// (4 MB for 32 CUs x 128-256 KB of output per tile) and push out the A panel / weight lines the neighbouring workgroups re-read.  Same box,
// s2 fc1 (us): bias 239.7 / 238.7 -> 225.1 / 228.4, + GELU 302.7 / 306.0 -> 289.2 / 289.5, GELU' 318.0 / 317.1 -> 315.8 / 311.7; whole step
// 147.2 -> 144.6 ms (HEAL-SWIN-B), 45.9 -> 44.7 ms (paper T @ 256); sc1 (write-through) alone: nothing (profiles/r06_gemm_store_policy.txt)
constexpr int kStoreAux = 2;
// Cache policy of the epilogue's INPUT rows (h for GELU', the residual), read once through the DMA ring.  2 = non-temporal,
// for the reason above: GELU' s2 292.0 / 293.5 -> 282.8 / 286.4 us, s1 426 / 423 -> 414 / 415 (profiles/r06_gemm_store_policy.txt)
constexpr int kInAux = 2;
enum { EPI_BIAS = 0, EPI_GELU = 1, EPI_DGELU = 2, EPI_RESID = 3 };
constexpr int64_t kMaxRecords = 0x7FFFFE00;  // descriptors are clamped to this many bytes (tiles address < 2 GiB from their origin)

struct GemmParams {
    const uint16_t *a, *b;
    int64_t lda, ldb;
    int k;
    const uint16_t *a2, *b2;
    int64_t lda2, ldb2;
    int k2;
    const float* bias;
    uint16_t* c;
    uint16_t* aux;
    int64_t m;
    int n;
    int tiles_n, tiles, per_xcd, blocks_per_xcd;
    float drop_p;
    uint64_t seed;
    HS_GEMM_TRACE_PARAM
};

// ---- tile traits: everything a tile variant determines.
// NSTAGE LDS stage buffers (the DMA runs NSTAGE - 1 k-steps ahead of the MFMAs); ALIAS: the epilogue's per-wave patches lie
// inside the stage buffer that was just consumed (one extra barrier per tile) instead of in LDS of their own
template <int BM_, int BN_, int WM_, int WN_, int NSTAGE_, bool ALIAS_, int WGS_PER_CU_>
struct TileTraits {
    static constexpr int BM = BM_, BN = BN_, WM = WM_, WN = WN_, NSTAGE = NSTAGE_, WGS_PER_CU = WGS_PER_CU_;
    static constexpr bool ALIAS = ALIAS_;
    static constexpr int NW = WM * WN;
    static constexpr int TM = BM / WM / 32, TN = BN / WN / 32;  // 32x32 accumulators per wave along m / n
    static constexpr int AB = BM * 128, BB = BN * 128, STAGE = AB + BB;
    static constexpr int AHEAD = NSTAGE - 1;
    // a wave's columns are one 64-wide patch pass of the epilogue; the fragment-read ring and its waits are written for TM = 2 and 4
    static_assert(TN == 2 && (TM == 2 || TM == 4), "the kernel is written for wave tiles of 64 columns and 64 or 128 rows");
    static_assert(!ALIAS || NW * 4096 <= STAGE, "patches do not fit a stage buffer");
    static_assert(BN * 4 <= 1024, "a bias slot holds one 1-KB DMA piece");

    static constexpr bool has_in(int epi) { return epi == EPI_DGELU || epi == EPI_RESID; }
    // RING: the epilogue's INPUT rows (h for GELU', the residual) of the 256 x 256 tile go global -> LDS by DMA through two patches
    // per wave inside the consumed stage buffer, requested two row blocks ahead and waited for by COUNT (the other tiles load them
    // into registers: one HBM round trip per row block behind a full vmcnt(0))
    static constexpr bool ring(int epi) { return has_in(epi) && ALIAS && TM == 4 && STAGE >= NW * 8192; }
    // LBIAS: the tile's BN bias values travel global -> LDS by one DMA piece of wave 0 when the ISSUE cursor enters the tile (1-KB
    // slots behind the stages) and the epilogue reads them with ds_read_b128.  A global load at the top of the
    // epilogue is the youngest entry of the wave's in-order vmcnt queue: on the DMA-issuing waves it waited for the whole first
    // k-step of the NEXT tile (64 KB from L2 / HBM) before row block 0 could start -- 3700 cycles per tile on the waves every
    // barrier then waits for (profiles/archive_r01_r04/r03_gemm_pass_overlap.txt: row block 0 8582 cycles on wave 0, 4878 on wave 7).
    // (Not on the 128 x 128 tile: its two workgroups per CU use all 160 KB already.)
    // Slot invariant: NSLOT = NSTAGE + 1 slots, taken by the workgroup's tile counter modulo NSLOT.  The bias of the tile that holds
    // k-step s + NSTAGE is issued in the iteration that computes step s, before that iteration's epilogue; a tile spans >= 1 k-step,
    // so the live tiles are the computed one and at most NSTAGE after it -- NSTAGE + 1 slots.  Tile T + NSLOT, the next user of T's
    // slot, starts >= NSLOT k-steps after T, so its bias is issued in an iteration after the one that ends with epilogue(T), behind
    // that iteration's barrier: every wave's ds_read of the slot has returned (lds_bias waits for lgkmcnt(0)).  With two slots by
    // parity, nk <= NSTAGE - 1 k-steps per tile let tile T + 2 overwrite T's bias before epilogue(T) (tests/test_gpu_gemm_stream.py).
    // Arrival: wave 0 issues a tile's bias piece right before the operand pieces of the tile's first k-step, in the same in-order
    // vmcnt queue; the main loop's wait for those pieces (before the barrier that precedes the step's MFMAs) covers the bias, so the
    // epilogue needs no wait of its own.
    static constexpr bool lbias(int epi) { return ALIAS && epi != EPI_DGELU; }
    static constexpr int NSLOT = NSTAGE + 1;
    // LDS layout: stages (+ epilogue patches of their own) (+ bias slots) (+ trace events)
    static constexpr int PATCH_OFF = NSTAGE * STAGE;  // (!ALIAS)
    static constexpr int BIAS_OFF = NSTAGE * STAGE + (ALIAS ? 0 : NW * 4096);
    static constexpr int bias_lds(int epi) { return lbias(epi) ? NSLOT * 1024 : 0; }
    static constexpr int trace_off(int epi) { return BIAS_OFF + bias_lds(epi); }
    static constexpr int lds_bytes(int epi) { return trace_off(epi) + trace_lds(trace_off(epi), NW); }
};
// The variants by their hs_gemm_nt_set_tile numbers: 1 = 128x128 x 2 stages, own epilogue patches, two 4-wave workgroups per CU;
// 2 = 256x128 x 3 stages and 3 = 256x256 x 2 stages: one 8-wave workgroup per CU, patches inside the consumed stage buffer
using Tile1 = TileTraits<128, 128, 2, 2, 2, false, 2>;
using Tile2 = TileTraits<256, 128, 4, 2, 3, true, 1>;
using Tile3 = TileTraits<256, 256, 2, 4, 2, true, 1>;

// Vector-memory instructions younger than the input request of row block i at the moment the epilogue waits for it.  Issue
// order: D_0, D_1, then per block b its 4 stores S_b and the 4 DMA instructions of D_{b+2} (loads and stores retire in order).
constexpr int epi_younger_ops(int tm, int i) {
    const int stores = i < 2 ? i : 1;
    const int last_d = i + 1 < tm - 1 ? i + 1 : tm - 1;
    return 4 * (stores + (last_d - i));
}

template <int OFF>
__device__ __forceinline__ u32x4 lds_read_b128(uint32_t addr) {
    u32x4 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}
constexpr int next_in_ring(int x, int n) { return x + 1 == n ? 0 : x + 1; }
__device__ __forceinline__ u32x2 pack_bf16x4(f32x2 lo, f32x2 hi) { return u32x2{pack_bf16x2(lo.x, lo.y), pack_bf16x2(hi.x, hi.y)}; }
__device__ __forceinline__ __amdgpu_buffer_rsrc_t clamped_rsrc(const void* ptr, int64_t bytes) {
    bytes = bytes > kMaxRecords ? kMaxRecords : bytes;
    return __builtin_amdgcn_make_buffer_rsrc((void*)ptr, 0, (int)bytes, 0x00020000);
}
// The wave's own operand pieces of the current k-step have landed once no more than `LATER` later pieces and `EPI_OPS` operations of
// an epilogue remain in its in-order queue, which holds, youngest last: [this step's pieces] [the later steps' pieces] [the
// epilogue's stores and input requests]
template <int LATER, int EPI_OPS>
__device__ __forceinline__ void wait_pieces_behind() {
    static_assert(LATER + EPI_OPS <= 63, "vmcnt immediate");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LATER + EPI_OPS) : "memory");
}

// ---- the DMA issue side of one operand (A or B): N 1-KB pieces per issuing wave and k-step, written LDS bytes in front of the
// operand inside a stage buffer.
// Lane mapping: LDS position q (16-B units inside a tile) = (super-row R = q / 16, physical chunk q % 16);
// logical chunk = physical ^ (R & 15); tile row = 2 R + (logical >> 3), 16-byte column chunk = logical & 7
// (SC, the scalar-offset form of FAST, keeps FOUR offsets whatever the piece count: pieces j and j + 4 of a wave differ by 32 tile
// rows and nothing else -- the swizzle term depends on j % 4 only -- and that part rides in the scalar offset together with k)
template <int N_, int LDS_, bool SC>
struct Operand {
    static constexpr int N = N_, LDS = LDS_, J = SC ? 4 : N;
    static_assert(N >= 1 && (!SC || N % 4 == 0), "FAST: whole groups of four pieces per issuing wave");
    __amdgpu_buffer_rsrc_t rsrc;
    int row[J], col[J];  // this lane's (tile row, byte column) of piece j
    int off[J];          // byte offset of this lane's (row, chunk) inside the tile, k-step 0
    int ld32 = 0;        // (SC) bytes of 32 operand rows
    __device__ __forceinline__ void map_lanes(int wave, int lane) {
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int q = (wave * N + j) * 64 + lane, R = q >> 4, lc = (q & 15) ^ (R & 15);
            row[j] = 2 * R + (lc >> 3);
            col[j] = (lc & 7) << 4;
        }
    }
    // the tile whose first row is row0 of `rows`, in the segment at `base` with rows of kseg bytes, ld elements apart
    __device__ __forceinline__ void retarget(const uint16_t* base, int64_t ld, int64_t row0, int64_t rows, int kseg) {
        rsrc = clamped_rsrc(base + row0 * ld, (rows - row0 - 1) * ld * 2 + kseg);
#pragma unroll
        for (int j = 0; j < J; ++j) off[j] = row[j] * ((int)ld * 2) + col[j];
        ld32 = (int)ld * 64;
    }
    // piece q of the k-step at byte kb of the row -> stage buffer `stage`
    __device__ __forceinline__ void issue(unsigned char* stage, int wave, int q, int kb, int kseg) const {
        lds_void* dst = (lds_void*)(stage + LDS + (wave * N + q) * 1024);
        if constexpr (SC) {
            // (k % 64 == 0: no K-tail predicate; the k offset and the 32-row group ride in the scalar operand, which takes
            // part in the descriptor's range check like the vector part)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, dst, 16, (uint32_t)off[q % J], kb + (q >> 2) * ld32, 0, 0);
        } else {
            const uint32_t voff = kb + col[q] < kseg ? (uint32_t)(off[q] + kb) : kOob;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, dst, 16, voff, 0, 0, 0);
        }
    }
};
// fragment address of operand row r (tile row), lane half h supplies k-chunk 2 ksub + h of the 16-deep MFMA step:
// byte = R * 256 + ((((r & 1) * 8 + 2 ksub + h) ^ (R & 15)) << 4) = frag_addr ^ (ksub << 5)
__device__ __forceinline__ uint32_t frag_addr(uint32_t lds_base, int r, int half) {
    const int R = r >> 1;
    return lds_base + R * 256 + (((((r & 1) << 3) + half) ^ (R & 15)) << 4);
}

// FAST (k and k2 multiples of 64: no K tail): the operand DMA of a k-step is issued by the FIRST HALF of the waves alone (twice the
// pieces each, their k offset in the scalar operand), the other half runs MFMAs and fragment reads only -- 8-16 % on the 256 x 256
// tile at every shape (profiles/archive_r01_r04/r03_gemm_role_split.txt); the addressing form alone changes nothing
template <typename Tile, int EPI, bool DROP, bool FAST>
__global__ void __launch_bounds__(Tile::NW * 64, 2) gemm_nt_kernel(GemmParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int BM = Tile::BM, BN = Tile::BN, WM = Tile::WM, WN = Tile::WN, NW = Tile::NW, TM = Tile::TM, TN = Tile::TN;
    constexpr int NSTAGE = Tile::NSTAGE, AHEAD = Tile::AHEAD, NSLOT = Tile::NSLOT, STAGE = Tile::STAGE, BIAS_OFF = Tile::BIAS_OFF;
    constexpr bool ALIAS = Tile::ALIAS, HAS_IN = Tile::has_in(EPI), RING = Tile::ring(EPI), LBIAS = Tile::lbias(EPI);
    constexpr int IW = FAST ? NW / 2 : NW;  // waves that issue the operand DMA
    using OperandA = Operand<Tile::AB / 1024 / IW, 0, FAST>;
    using OperandB = Operand<Tile::BB / 1024 / IW, Tile::AB, FAST>;
    constexpr int PIECES = OperandA::N + OperandB::N;  // 1-KB DMA instructions per issuing wave and k-step
    static_assert(Tile::lds_bytes(EPI) <= 163840, "LDS of one workgroup exceeds 160 KB");
    __shared__ __attribute__((aligned(16))) unsigned char smem[Tile::lds_bytes(EPI)];

    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;

    // ---- this workgroup's tiles: XCD x owns ids [x * per_xcd, (x + 1) * per_xcd), dealt round-robin to its workgroups
    const int xcd = blockIdx.x & 7, lb = blockIdx.x >> 3;
    const int id_end = min((xcd + 1) * p.per_xcd, p.tiles);
    const int id0 = xcd * p.per_xcd + lb;
    if (id0 >= id_end) return;
    const int nk1 = (p.k + 63) >> 6, nk2 = (p.k2 + 63) >> 6, nk = nk1 + nk2;
    struct Origin {
        int64_t m0;
        int n0;
    };
    auto tile_origin = [&](int id) {
        const int tm = id / p.tiles_n, tn = id - tm * p.tiles_n;
        return Origin{(int64_t)tm * BM, tn * BN};
    };

    // ---- issue side: the (tile, K segment) the DMA currently reads from.  Descriptors, row offsets and the row length are
    // rebuilt only when the issue cursor enters a new tile or segment, not per k-step.
    OperandA opa;
    OperandB opb;
    opa.map_lanes(wave, lane);
    opb.map_lanes(wave, lane);
    int kseg = 0;    // bytes of a row of the current segment
    int slot_i = 0;  // (LBIAS) slot the next tile's bias goes to
    __amdgpu_buffer_rsrc_t rbias = __builtin_amdgcn_make_buffer_rsrc((void*)p.bias, 0, p.bias ? p.n * 4 : 0, 0x00020000);
    auto retarget = [&](int id, bool s2, bool enter) {
        const Origin o = tile_origin(id);
        if constexpr (LBIAS) {
            if (enter) {
                // lanes beyond the tile's BN floats (and columns beyond n) read outside the descriptor: zeros
                if (wave == 0)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rbias, (lds_void*)(smem + BIAS_OFF + slot_i * 1024), 16,
                                                             lane * 4 < BN ? (uint32_t)(lane * 16) : kOob, o.n0 * 4, 0, 0);
                slot_i = next_in_ring(slot_i, NSLOT);
            }
        }
        // (copies first: with `s2 ? p.lda2 : p.lda` written as the call's argument the compiler selected between the ADDRESSES of the
        // kernel arguments, which it then kept in scratch -- 40 bytes per lane and 5-10 VGPRs more in every kernel)
        const uint16_t* ap = s2 ? p.a2 : p.a;
        const uint16_t* bp = s2 ? p.b2 : p.b;
        const int64_t lda = s2 ? p.lda2 : p.lda, ldb = s2 ? p.ldb2 : p.ldb;
        kseg = (s2 ? p.k2 : p.k) * 2;
        opa.retarget(ap, lda, o.m0, p.m, kseg);
        opb.retarget(bp, ldb, o.n0, p.n, kseg);
    };
    // DMA pieces [first, first + count) of the PIECES pieces of one k-step (byte offset kb inside the row) into stage `buf`
    auto issue_pieces = [&](int kb, int buf, auto first_c, auto count_c) {
        constexpr int first = decltype(first_c)::value, count = decltype(count_c)::value;
        if (IW < NW && wave >= IW) return;
        unsigned char* base = smem + buf * STAGE;
#pragma unroll
        for (int q = first; q < first + count; ++q) {
            if (q < OperandA::N) opa.issue(base, wave, q, kb, kseg);
            else opb.issue(base, wave, q - OperandA::N, kb, kseg);
        }
    };

    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    Trace TR(p, Tile::lds_bytes(EPI) > Tile::trace_off(EPI), lds0 + Tile::trace_off(EPI), NW, wave, lane);
    uint32_t a_frag[TM], b_frag[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) a_frag[i] = frag_addr(lds0 + OperandA::LDS, wm * (BM / WM) + i * 32 + l31, half);
#pragma unroll
    for (int j = 0; j < TN; ++j) b_frag[j] = frag_addr(lds0 + OperandB::LDS, wn * (BN / WN) + j * 32 + l31, half);

    f32x16 acc[TN][TM];
    zero(acc);

    // ---- one k-step out of stage buffer `buf`: four 16-deep MFMA sub-steps, their fragment reads streamed ahead of them, and
    // the DMA pieces of a later k-step (into stage buffer `buf_next`, free since the barrier) issued behind each MFMA group
    auto compute = [&](int buf, bool prefetch, int kb_next, int buf_next) {
        const uint32_t bo = buf * STAGE;
        // fragment reads are streamed one or two 16-deep sub-steps ahead of their MFMAs through a ring of NSET register sets
        // (two for the 128 x 64 wave tile, whose 128 accumulator registers leave no room for a third)
        constexpr int NSET = TM == 4 ? 2 : 3;
        u32x4 fa[NSET][TM], fb[NSET][TN];
        auto read_frags = [&](auto ks_c) {
            constexpr int ks = decltype(ks_c)::value, set = ks % NSET;
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[set][j] = lds_read_b128<0>((b_frag[j] ^ (ks << 5)) + bo);
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[set][i] = lds_read_b128<0>((a_frag[i] ^ (ks << 5)) + bo);
        };
        auto wait_frags = [&](auto ks_c, auto left_c) {
            constexpr int ks = decltype(ks_c)::value, left = decltype(left_c)::value, set = ks % NSET;
            (void)fa;  // (named outside the if-constexpr branches: clang otherwise refuses the implicit capture)
            (void)fb;
            // reads of sub-step ks have landed once at most `left` later reads are outstanding (LDS returns in order)
            if constexpr (TM == 2)
                asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(fa[set][0]), "+v"(fa[set][1]), "+v"(fb[set][0]), "+v"(fb[set][1]) : "n"(left));
            else
                asm volatile("s_waitcnt lgkmcnt(%6)"
                             : "+v"(fa[set][0]), "+v"(fa[set][1]), "+v"(fa[set][2]), "+v"(fa[set][3]), "+v"(fb[set][0]), "+v"(fb[set][1])
                             : "n"(left));
        };
        // MFMAs of sub-step ks, then DMA pieces [first, first + cnt) of a later step in their shadow
        auto mma = [&](auto ks_c, auto first_c, auto cnt_c) {
            constexpr int ks = decltype(ks_c)::value, set = ks % NSET;
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                        acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fb[set][j]),
                                                                            __builtin_bit_cast(bf16x8, fa[set][i]), acc[j][i], 0, 0, 0);
                }
            if (decltype(cnt_c)::value > 0 && prefetch) issue_pieces(kb_next, buf_next, first_c, cnt_c);
            __builtin_amdgcn_sched_barrier(0);
        };
        constexpr int PQ = (PIECES + 3) / 4;  // a quarter of the next free buffer's pieces behind each MFMA group
        read_frags(Int<0>{});
        read_frags(Int<1>{});
        static_for<4>([&](auto ks_c) {
            constexpr int ks = decltype(ks_c)::value;
            constexpr int rest = PIECES - ks * PQ, cnt = rest < 0 ? 0 : rest < PQ ? rest : PQ;
            wait_frags(ks_c, Int<(ks < 3 ? TM + TN : 0)>{});  // (outstanding behind it: the reads of sub-step ks + 1)
            mma(ks_c, Int<ks * PQ>{}, Int<cnt>{});
            if constexpr (ks + 2 < 4) read_frags(Int<ks + 2>{});  // re-uses the set of a group whose MFMAs have all been issued
        });
    };

    // ---- epilogue of tile `id`.  A lane owns output row m = l31 of each 32-row block and 4 consecutive n per register group.
    // Row-per-lane 8-byte global stores touch 32 cache lines per instruction and are issue-bound (16 of them per lane cost
    // thousands of cycles), so each wave passes its [32 rows][64 columns] block through a private 4 KB LDS patch
    // (16-byte chunk ^ (row & 7): the 8-byte writes are 2-way, the 16-byte reads conflict-free) and stores / loads WHOLE
    // 128-byte row segments: 4 dwordx4 instructions per block, 8 rows each.  All patch accesses are inline asm: a
    // compiler-visible LDS access beside the DMA queue would be preceded by s_waitcnt vmcnt(0) and stall the epilogue
    // behind the next tile's first loads.  Needs n % 8 == 0; otherwise (the 12-class head) the direct 8-byte form is used.
    const uint32_t own_rel = wave * 4096 + l31 * 128 + 8 * half;     // + ((chunk ^ (l31 & 7)) << 4), chunk = 4 j + g
    // OUTPUT blocks are written with the two 8-byte halves of every 16-byte chunk exchanged in rows 8-15 and 24-31: rows r and r + 8
    // of a 16-lane ds_write_b64 group share chunk slot and half otherwise (2-way conflict on every patch write: 1540 instead of
    // 770 LDS cycles per row block and CU); the row view undoes it for free -- its row is lane / 8 + 8 t, so bit 3 is t & 1 and the
    // odd t swap register halves
    const uint32_t own_out_rel = wave * 4096 + l31 * 128 + 8 * (half ^ ((l31 >> 3) & 1));
    const uint32_t row_rel = wave * 4096 + (lane >> 3) * 128 + (((lane & 7) ^ (lane >> 3)) << 4);  // + t * 1024: row lane/8 + 8 t
    // (dropout) whether the lane's four consecutive elements are the SECOND half of a generator chunk.  Their element index is
    // row * n + column; the column is 4 * half modulo 8, and with n % 8 == 4 the odd rows begin in the middle of a chunk -- the odd
    // lanes, since every row block begins at an even row.  A lane constant (the lane half alone gave the odd rows of such an n the
    // other half's multipliers: not the mask hs_gelu_fwd draws, tests/test_gpu_gemm.py)
    const bool second_half = ((half ^ (lane & (p.n >> 2))) & 1) != 0;
    auto epilogue = [&](int id, int buf_done, int slot_c) {
        const uint32_t patch_off = ALIAS ? buf_done * STAGE : Tile::PATCH_OFF;  // byte offset of the patch area inside smem
        TR(10);
        if (ALIAS) __builtin_amdgcn_s_barrier();  // every wave is done reading the stage buffer the patches live in
        TR(11);
        const Origin o = tile_origin(id);
        const int64_t m0 = o.m0;
        const int n2 = p.n * 2;
        const int64_t cbytes = (p.m - m0) * (int64_t)n2;
        const __amdgpu_buffer_rsrc_t rc = clamped_rsrc(p.c + m0 * p.n, p.c ? cbytes : 0);
        const __amdgpu_buffer_rsrc_t rx = clamped_rsrc(p.aux + m0 * p.n, p.aux ? cbytes : 0);
        const ElemRng rng(p.drop_p, p.seed);
        const bool wide = RING || (p.n & 7) == 0;  // whole-row-segment path
        const int ncol0 = o.n0 + wn * (BN / WN);    // first of the wave's 64 columns
        // the lane's first column of register group g of accumulator j
        auto col_of = [&](int j, int g) { return ncol0 + j * 32 + 4 * half + 8 * g; };
        float4 bias4[TN][4];
        // (LBIAS: a column block's four float4 are read from the LDS slot where they are used -- 4 broadcast reads per block instead of
        // 32 registers held across the pass, which the RESID epilogue of the 128 x 64 wave tile does not have)
        const uint32_t baddr = lds0 + BIAS_OFF + slot_c * 1024 + (wn * (BN / WN) + 4 * half) * 4;
        auto lds_bias = [&](int j, float4 (&b)[4]) {
            u32x4 bq[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) asm volatile("ds_read_b128 %0, %1" : "=v"(bq[g]) : "v"(baddr + (j * 32 + 8 * g) * 4));
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(bq[0]), "+v"(bq[1]), "+v"(bq[2]), "+v"(bq[3]));
#pragma unroll
            for (int g = 0; g < 4; ++g) b[g] = __builtin_bit_cast(float4, bq[g]);
        };
        if constexpr (!LBIAS) {
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int n = col_of(j, g);
                    bias4[j][g] = (EPI != EPI_DGELU && p.bias && n < p.n) ? *(const float4*)(p.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
        }
        // row-lane view of a block: lane -> (row lane/8 + 8 t, 16-byte chunk lane % 8).  The per-lane part of the byte offset is ONE
        // register; the row block / row group part is wave-uniform and rides in the instruction's scalar offset (it takes part
        // in the descriptor's range check like the vector part).  Per-(i, t) vector offsets were hoisted out of the tile loop
        // by the compiler and spilled: every reload inside the store sequence is a `s_waitcnt vmcnt(0)`, i.e. a full drain of
        // the stores issued so far -- two of them cost the bias epilogue 5000 cycles per tile (tools/gemm_trace.py)
        const int rl_col = ncol0 + (lane & 7) * 8;
        const uint32_t rl_voff = rl_col < p.n ? (uint32_t)((lane >> 3) * n2 + rl_col * 2) : kOob;
        auto row_soff = [&](int i, int t) -> int { return (wm * (BM / WM) + i * 32 + 8 * t) * n2; };
        // input ring: row block i passes through patch slot i % 2 (slot s of wave w at patch_off + s * NW * 4096 + w * 4096).  A DMA
        // lane writes LDS position lane * 16 of its 1-KB piece = (row lane / 8, physical chunk lane % 8), so it FETCHES logical
        // chunk (lane % 8) ^ (lane / 8) of that row: the image the own-lane reads expect, every 128-byte row segment still one
        // request of 8 adjacent lanes.  (Launched only with n % 8 == 0: gemm_nt_tile_variant.)
        const int in_col = ncol0 + (((lane & 7) ^ (lane >> 3)) << 3);
        const uint32_t in_voff = in_col < p.n ? (uint32_t)((lane >> 3) * n2 + in_col * 2) : kOob;
        auto request_in = [&](int i) {
            unsigned char* base = smem + patch_off + (i & 1) * (NW * 4096) + wave * 4096;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_void*)(base + t * 1024), 16, in_voff, row_soff(i, t), 0, kInAux);
        };
        if constexpr (RING) {
            request_in(0);
            request_in(1);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int ml = wm * (BM / WM) + i * 32 + l31;
            // the lane's own 8 bytes (global byte offset inside the tile's rows) in the direct 8-byte form
            auto direct_off = [&](int j, int g) { return col_of(j, g) < p.n ? (uint32_t)(ml * n2 + col_of(j, g) * 2) : kOob; };
            // ---- input block (h or the residual) in the own-lane view
            const uint32_t pbase = lds0 + patch_off + (RING ? (i & 1) * (NW * 4096) : 0);
            const uint32_t own_addr = pbase + own_rel, row_addr = pbase + row_rel, own_out = pbase + own_out_rel;
            u32x2 xin[TN][4];
            if (HAS_IN) {
                if (wide) {
                    if constexpr (RING) {
                        // this block's rows have landed once only the younger operations are outstanding
                        static_for<TM>([&](auto b) {
                            if (i == b) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(epi_younger_ops(TM, b)) : "memory");
                        });
                    } else {
                        u32x4 rws[4];
#pragma unroll
                        for (int t = 0; t < 4; ++t)
                            rws[t] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, rl_voff, row_soff(i, t), 0));
                        asm volatile("ds_write_b128 %0, %1" ::"v"(row_addr), "v"(rws[0]) : "memory");
                        asm volatile("ds_write_b128 %0, %1 offset:1024" ::"v"(row_addr), "v"(rws[1]) : "memory");
                        asm volatile("ds_write_b128 %0, %1 offset:2048" ::"v"(row_addr), "v"(rws[2]) : "memory");
                        asm volatile("ds_write_b128 %0, %1 offset:3072" ::"v"(row_addr), "v"(rws[3]) : "memory");
                    }
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int g = 0; g < 4; ++g)
                            asm volatile("ds_read_b64 %0, %1" : "=v"(xin[j][g]) : "v"(own_addr + (((4 * j + g) ^ (l31 & 7)) << 4)));
                    asm volatile("s_waitcnt lgkmcnt(0)"
                                 : "+v"(xin[0][0]), "+v"(xin[0][1]), "+v"(xin[0][2]), "+v"(xin[0][3]), "+v"(xin[1][0]),
                                   "+v"(xin[1][1]), "+v"(xin[1][2]), "+v"(xin[1][3]));
                } else {
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int g = 0; g < 4; ++g) xin[j][g] = __builtin_amdgcn_raw_buffer_load_b64(rx, direct_off(j, g), 0, 0);
                }
            }
            // dropout: the lane's four consecutive elements are the first or the second half of a chunk of the generator
            // (hs_device.h): one chunk key, one multiply per element pair, formed where the pair is used
            auto chunk_key = [&](int j, int g) { return rng.chunk_key((uint64_t)((m0 + ml) * p.n + col_of(j, g)) >> 3); };
            auto keep2 = [&](uint32_t ck, int t) {
                const uint32_t hh = ElemRng::pair_bits(ck, ElemRng::half_mult(second_half, t));
                return f32x2{rng.keep_lo(hh), rng.keep_hi(hh)};
            };
            // ---- arithmetic on the accumulators, two elements at a time (packed fp32, hs_gelu.h).  Dropout (DROP) is a
            // kernel instantiation of its own: next to the branch-free p = 0 arithmetic its counter hashes cost the
            // 128 x 64 wave tile ~70 spilled registers, some of them inside the main loop
            u32x2 o1[TN][4], o2[TN][4];  // o1 -> c ; o2 -> aux (EPI_GELU only)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                if constexpr (LBIAS) lds_bias(j, bias4[j]);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x16& a16 = acc[j][i];
                    f32x2 v[2] = {f32x2{a16[4 * g], a16[4 * g + 1]} + f32x2{bias4[j][g].x, bias4[j][g].y},
                                  f32x2{a16[4 * g + 2], a16[4 * g + 3]} + f32x2{bias4[j][g].z, bias4[j][g].w}};
                    uint32_t ck = 0;
                    if (DROP) ck = chunk_key(j, g);
                    if (EPI == EPI_GELU) {
                        // h is packed here and kept (fp32) in the accumulator registers; the activation is computed from them
                        // by make_o2 below, at the place in the block's sequence that the wave's role asks for
                        o1[j][g] = pack_bf16x4(v[0], v[1]);
                        a16[4 * g] = v[0].x; a16[4 * g + 1] = v[0].y; a16[4 * g + 2] = v[1].x; a16[4 * g + 3] = v[1].y;
                        continue;
                    } else {
                        if (EPI == EPI_DGELU || EPI == EPI_RESID) {
#pragma unroll
                            for (int t = 0; t < 2; ++t) {
                                const f32x2 x = {__uint_as_float(xin[j][g][t] << 16), __uint_as_float(xin[j][g][t] & 0xffff0000u)};
                                if (EPI == EPI_DGELU) {
                                    v[t] *= gelu_grad2(x);
                                    if (DROP) v[t] *= keep2(ck, t);
                                } else {
                                    v[t] += x;
                                }
                            }
                        }
                        o1[j][g] = pack_bf16x4(v[0], v[1]);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) a16[4 * g + r] = 0.f;
                }
            }
            auto make_o2 = [&]() {  // (EPI_GELU) aux = dropout(gelu(h)); clears the accumulators.  Four element pairs in lock step.
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int g0 = 0; g0 < 4; g0 += 2) {
                        f32x16& a16 = acc[j][i];
                        f32x2 v[4] = {f32x2{a16[4 * g0], a16[4 * g0 + 1]}, f32x2{a16[4 * g0 + 2], a16[4 * g0 + 3]},
                                      f32x2{a16[4 * g0 + 4], a16[4 * g0 + 5]}, f32x2{a16[4 * g0 + 6], a16[4 * g0 + 7]}};
                        // (four pairs in lock step, gelu2_n<4>, measured: no faster -- the block is bound by its patch round trips
                        // and store issue, not by the chains' latency; profiles/r06_gemm_epilogue_experiments.txt)
#pragma unroll
                        for (int t = 0; t < 4; ++t) v[t] = gelu2(v[t]);
#pragma unroll
                        for (int gg = 0; gg < 2; ++gg) {
                            const int g = g0 + gg;
                            if (DROP) {
                                const uint32_t ck = chunk_key(j, g);
#pragma unroll
                                for (int t = 0; t < 2; ++t) v[2 * gg + t] *= keep2(ck, t);
                            }
                            o2[j][g] = pack_bf16x4(v[2 * gg], v[2 * gg + 1]);
#pragma unroll
                            for (int r = 0; r < 4; ++r) a16[4 * g + r] = 0.f;
                        }
                    }
            };
            TR(20);  // arithmetic of the block done
            // ---- outputs
            auto emit = [&](const __amdgpu_buffer_rsrc_t& rs, const u32x2 (&o)[TN][4]) {
                if (wide) {
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int g = 0; g < 4; ++g)
                            asm volatile("ds_write_b64 %0, %1" ::"v"(own_out + (((4 * j + g) ^ (l31 & 7)) << 4)), "v"(o[j][g]) : "memory");
                    u32x4 rws[4];
                    // (rows 8-15 / 24-31 of the block = odd t: the chunk halves lie exchanged, own_out_rel -- ds_read2_b64 with the
                    // two 8-byte offsets in reverse order returns them in place.  NOT a register swap after the read: hipcc put the
                    // four v_mov straight behind the buffer_store_dwordx4 of the previous row group, over its data registers, and
                    // lanes 12-15 of every 16 stored the NEW first dword (no hazard is listed for a store with an SGPR offset,
                    // none is inserted; seen on gfx950 / ROCm 7.2, tests/test_gpu_gemm.py caught it))
                    asm volatile("ds_read_b128 %0, %1" : "=v"(rws[0]) : "v"(row_addr));
                    asm volatile("ds_read2_b64 %0, %1 offset0:129 offset1:128" : "=v"(rws[1]) : "v"(row_addr));
                    asm volatile("ds_read_b128 %0, %1 offset:2048" : "=v"(rws[2]) : "v"(row_addr));
                    asm volatile("ds_read2_b64 %0, %1 offset0:129 offset1:128" : "=v"(rws[3]) : "v"(row_addr + 2048));
                    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(rws[0]), "+v"(rws[1]), "+v"(rws[2]), "+v"(rws[3]));
                    TR(22);  // patch round trip done
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, rws[t]), rs, rl_voff, row_soff(i, t), kStoreAux);
                    // the data registers stay live across one wait state behind the last store (see above)
                    asm volatile("s_nop 0" ::"v"(rws[0]), "v"(rws[1]), "v"(rws[2]), "v"(rws[3]));
                } else {
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int g = 0; g < 4; ++g) __builtin_amdgcn_raw_buffer_store_b64(o[j][g], rs, direct_off(j, g), 0, kStoreAux);
                }
            };
            if (EPI == EPI_GELU) {
                // The two waves of a SIMD (w and w + NW / 2) take the outputs in OPPOSITE order: the GELU arithmetic is bound by the
                // SIMD's VALU rate (~770 cycles per block and wave alone, twice that when both partners are in it), the h output is
                // LDS patch + store issue (~1100) -- out of phase each hides under the other (tools/gemm_trace.py,
                // profiles/r06_gemm_trace_epilogue_phases.txt)
                if (NW == 8 && wave >= NW / 2) {
                    make_o2();
                    emit(rx, o2);
                    TR(21);
                    __builtin_amdgcn_sched_barrier(0);
                    if (p.c) emit(rc, o1);
                } else {
                    if (p.c) emit(rc, o1);
                    TR(21);  // first output's stores issued
                    __builtin_amdgcn_sched_barrier(0);
                    make_o2();
                    emit(rx, o2);
                }
            } else {
                emit(rc, o1);
            }
            if constexpr (RING) {
                if (i + 2 < TM) request_in(i + 2);  // the patch is free again: its rows are in registers
            }
            TR(12 + i);
        }
    };

    // ---- the stream of k-steps over this workgroup's tiles; the issue cursor runs NSTAGE - 1 steps ahead of the compute cursor
    const int stride = p.blocks_per_xcd;
    int id_i = id0, ks_i = 0;  // next step to issue
    int id_c = id0, ks_c = 0;  // step being computed
    int slot_c = 0;            // (LBIAS) slot that holds the bias of the tile being computed
    auto advance_issue = [&]() {
        ++ks_i;
        if (ks_i == nk) {
            ks_i = 0;
            id_i += stride;
            if (id_i < id_end) retarget(id_i, nk1 == 0, true);
        } else if (ks_i == nk1) {
            retarget(id_i, true, false);
        }
    };
    auto kb_of = [&](int ks) { return (ks >= nk1 ? ks - nk1 : ks) * 128; };
    retarget(id_i, false, true);
    int issued = 0;  // steps issued and not yet computed
#pragma unroll
    for (int q = 0; q < AHEAD; ++q) {
        if (id_i < id_end) {
            issue_pieces(kb_of(ks_i), q, Int<0>{}, Int<PIECES>{});
            advance_issue();
            ++issued;
        }
    }
    int buf = 0, buf_free = AHEAD;  // buffer being computed; buffer the next issue goes to
    bool drained = false;           // an epilogue's stores are in the queue behind the operand pieces
    constexpr int LATER = (AHEAD - 1) * PIECES;  // pieces of the later steps allowed in flight
    constexpr int kEpiOps = TM * 4;  // vector-memory operations of the SMALLEST epilogue (four row-segment stores per row block)
    TR(0);
    while (true) {
        TR(3);
        // this wave's loads of the current step have landed: everything older than the steps still allowed in flight
        if (IW < NW && wave >= IW) {
            // (this wave issues no operand DMA -- nothing of its own to wait for; its epilogue stores are fire-and-forget, and
            // an epilogue waits for its own input loads itself)
        } else if (AHEAD > 1 && issued == AHEAD && !drained)
            wait_pieces_behind<LATER, 0>();
        else if (drained && issued == AHEAD)
            // behind an epilogue, waiting for the STORES' acknowledgements (vmcnt(0)) cost the issuing waves -- the ones every barrier
            // waits for -- ~700 cycles per tile (tools/gemm_trace.py: "epilogue end -> next step"); the pieces are covered once no more
            // than the later steps' pieces and kEpiOps epilogue operations remain (kEpiOps = the fewest an epilogue issues: one
            // output's stores)
            wait_pieces_behind<LATER, kEpiOps>();
        else if (drained && issued == 1)
            wait_pieces_behind<0, kEpiOps>();
        else
            wait_pieces_behind<0, 0>();
        drained = false;
        TR(1);
        __builtin_amdgcn_s_barrier();  // ... everyone's have; and everyone is done reading the buffer that is re-filled next
        TR(2);
        const bool more = id_i < id_end;
        const bool last = ks_c + 1 == nk;
        compute(buf, more, kb_of(ks_i), buf_free);
        --issued;
        if (more) {
            advance_issue();
            ++issued;
        }
        const int buf_done = buf;
        buf = next_in_ring(buf, NSTAGE);
        buf_free = next_in_ring(buf_free, NSTAGE);
        if (last) {
            epilogue(id_c, buf_done, slot_c);
            slot_c = next_in_ring(slot_c, NSLOT);
            drained = true;
            ks_c = 0;
            id_c += stride;
            if (id_c >= id_end) break;
        } else {
            ++ks_c;
        }
    }
    TR.flush();
#endif
}

template <typename Tile, bool FAST>
int launch_tile(GemmParams& p, int epi, hipStream_t s) {
    const int tiles_m = (int)((p.m + Tile::BM - 1) / Tile::BM);
    p.tiles_n = (p.n + Tile::BN - 1) / Tile::BN;
    const int64_t tiles = (int64_t)tiles_m * p.tiles_n;
    if (tiles > 0x7fffffff) return fail(HS_ERR_UNSUPPORTED, "too many output tiles");
    p.tiles = (int)tiles;
    p.per_xcd = (p.tiles + 7) / 8;
    const int resident = usable_cus_per_xcd() * Tile::WGS_PER_CU;  // workgroups per XCD in one resident round (32 CUs per XCD minus the reserved ones)
    p.blocks_per_xcd = p.per_xcd < resident ? p.per_xcd : resident;
    const dim3 grid((unsigned)(8 * p.blocks_per_xcd)), block(Tile::NW * 64);
    // [epilogue][drop_p > 0]: the bias and residual epilogues draw no mask
    using Kernel = void (*)(GemmParams);
    static constexpr Kernel kKernels[4][2] = {
        {gemm_nt_kernel<Tile, EPI_BIAS, false, FAST>, gemm_nt_kernel<Tile, EPI_BIAS, false, FAST>},
        {gemm_nt_kernel<Tile, EPI_GELU, false, FAST>, gemm_nt_kernel<Tile, EPI_GELU, true, FAST>},
        {gemm_nt_kernel<Tile, EPI_DGELU, false, FAST>, gemm_nt_kernel<Tile, EPI_DGELU, true, FAST>},
        {gemm_nt_kernel<Tile, EPI_RESID, false, FAST>, gemm_nt_kernel<Tile, EPI_RESID, false, FAST>}};
    hipLaunchKernelGGL(kKernels[epi][p.drop_p > 0.f], grid, block, 0, s, p);
    HS_LAUNCH_CHECK("gemm_nt");
    return HS_OK;
}

}  // namespace

int gemm_nt_check_shape(const char* who, int64_t lda, int64_t ldb, int k, int64_t lda2, int64_t ldb2, int k2, int64_t m, int n) {
    HS_CHECK_ARG(m > 0 && n > 0 && k > 0 && k2 >= 0, "%s: empty shape", who);
    // 16-byte operand chunks and 8-byte output groups
    if (k % 8 || k2 % 8 || lda % 8 || ldb % 8 || (k2 && (lda2 % 8 || ldb2 % 8)) || n % 4)
        return fail(HS_ERR_UNSUPPORTED, "%s: k, k2 and the row strides must be multiples of 8, n a multiple of 4", who);
    if (lda * 2 * 256 > kMaxRecords || ldb * 2 * 256 > kMaxRecords || (int64_t)n * 2 * 256 > kMaxRecords)
        return fail(HS_ERR_UNSUPPORTED, "%s: row stride too large", who);
    // (the 128 x 128 tile has the most tiles; launch_tile counts those of the tile it launches)
    if (((m + 127) / 128) * (((int64_t)n + 127) / 128) > 0x7fffffff) return fail(HS_ERR_UNSUPPORTED, "%s: too many output tiles", who);
    return HS_OK;
}

// The tile variant (Tile1 / Tile2 / Tile3) a product launches; `forced` != 0 (hs_gemm_nt_set_tile, for A/B runs) replaces the choice.
// Measured choice (tools/bench_gemm_nt.py, profiles/archive_r01_r04/r02_gemm_nt_vs_library.*): 256x128 x 3 is the all-round shape;
// 256x256 halves the L2 -> LDS fill per flop and wins wide outputs with k >= 512 and every GELU / GELU' epilogue with n >= 512 (fewer,
// larger tiles: the VALU-bound epilogue is paid per output element, the barrier / drain around it per tile);
// 128x128 when the launch would not fill the chip otherwise.
int gemm_nt_tile_variant(int forced, int64_t m, int n, int k, int k2, int epilogue) {
    int variant = forced;
    if (!variant) {
        const int64_t tiles2 = ((m + 255) / 256) * ((n + 127) / 128), tiles3 = ((m + 255) / 256) * ((n + 255) / 256);
        if (tiles2 < 256)
            variant = 1;
        else if ((epilogue == EPI_GELU || epilogue == EPI_DGELU) ? n >= 512 : (n >= 1024 && k + k2 >= 512))
            variant = 3;
        else if (n >= 256 && tiles3 >= 768 && k % 64 == 0 && k2 % 64 == 0)
            // with the role-separated DMA issue (FAST) the 256 x 256 tile also wins the narrower outputs (profiles/
            // r03_gemm_role_split.txt: s0 qkv 365 vs 392 us, s1 qkv 207 vs 258, s2 proj 60 vs 66) as long as its tiles
            // fill three resident rounds (stage-3 proj / fc2, 384 tiles = 1.5 rounds, stay on the 256 x 128 tile)
            variant = 3;
        else
            variant = 2;
    }
    // (the 256 x 256 kernels take an epilogue input through the DMA ring, which moves whole 16-byte chunks)
    if (variant == 3 && (epilogue == EPI_DGELU || epilogue == EPI_RESID) && n % 8) variant = 2;
    return variant == 2 || variant == 3 ? variant : 1;
}

}  // namespace hs

namespace {
int g_tile_variant = 0;  // hs_gemm_nt_set_tile (measurement hook): 1 = 128x128, 2 = 256x128, 3 = 256x256; 0 = heuristic
}

extern "C" {

int hs_gemm_nt_set_tile(int variant) {
    g_tile_variant = variant;
    return HS_OK;
}

int hs_gemm_nt_tile_variant(int64_t m, int n, int k, int k2, int epilogue) {
    return hs::gemm_nt_tile_variant(g_tile_variant, m, n, k, k2, epilogue);
}

int hs_gemm_nt(const void* a, int64_t lda, const void* b, int64_t ldb, int k, const void* a2, int64_t lda2, const void* b2,
               int64_t ldb2, int k2, const float* bias, void* c, void* aux, int64_t m, int n, int epilogue, float drop_p,
               uint64_t seed, int dtype, void* stream) {
    using namespace hs;
    HS_CHECK_ARG(dtype == HS_BF16, "hs_gemm_nt: bf16 activations only (fp32 runs use the library GEMM)");
    HS_CHECK_ARG(a && b && m > 0 && n > 0 && k > 0, "hs_gemm_nt: null operand or empty shape");
    HS_CHECK_ARG(epilogue >= EPI_BIAS && epilogue <= EPI_RESID, "hs_gemm_nt: unknown epilogue %d", epilogue);
    HS_CHECK_ARG(k2 == 0 || (a2 && b2 && k2 > 0), "hs_gemm_nt: second segment needs a2, b2, k2 > 0");
    HS_CHECK_ARG(c || (epilogue == EPI_GELU && aux), "hs_gemm_nt: no output");
    HS_CHECK_ARG(epilogue == EPI_BIAS || aux, "hs_gemm_nt: this epilogue needs aux");
    HS_CHECK_ARG(drop_p >= 0.f && drop_p <= 1.f, "hs_gemm_nt: drop_p must be in [0, 1]");
    HS_CHECK_ALIGNED("hs_gemm_nt", 16, a, b, a2, b2, bias, c, aux);  // operands and bias travel as 16-byte buffer-to-LDS chunks
    if (int st = gemm_nt_check_shape("hs_gemm_nt", lda, ldb, k, lda2, ldb2, k2, m, n)) return st;
    GemmParams p{};
    p.a = (const uint16_t*)a; p.b = (const uint16_t*)b; p.lda = lda; p.ldb = ldb; p.k = k;
    p.a2 = (const uint16_t*)a2; p.b2 = (const uint16_t*)b2; p.lda2 = lda2; p.ldb2 = ldb2; p.k2 = k2;
    p.bias = bias; p.c = (uint16_t*)c; p.aux = (uint16_t*)aux; p.m = m; p.n = n;
    p.drop_p = drop_p; p.seed = seed;
    trace_attach(p);
    hipStream_t st = (hipStream_t)stream;
    // role-separated DMA issue (FAST) wherever there is no K tail (8-16 % on the 256 x 256 tile, profiles/archive_r01_r04/r03_gemm_role_split.txt)
    const bool fast = k % 64 == 0 && k2 % 64 == 0;
    switch (gemm_nt_tile_variant(g_tile_variant, m, n, k, k2, epilogue)) {
        case 2: return fast ? launch_tile<Tile2, true>(p, epilogue, st) : launch_tile<Tile2, false>(p, epilogue, st);
        case 3: return fast ? launch_tile<Tile3, true>(p, epilogue, st) : launch_tile<Tile3, false>(p, epilogue, st);
        default: return launch_tile<Tile1, false>(p, epilogue, st);
    }
}

}  // extern "C"
