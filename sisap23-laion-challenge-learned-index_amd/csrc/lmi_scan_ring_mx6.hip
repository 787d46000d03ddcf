// scan3_mx6_kernel: the 8-wave ring on the MXFP6 codes of the 6-bit storage
// (LMI_MX6 / LMI_Q_MX6, include/lmi_hip.h "the MXFP6 format"), d_pad == 768,
// plain lists of 10 or 16 entries.  The family ScanKernel::Ring8MX6 of the
// scan's plan.  Products run on v_mfma_scale_f32_32x32x64_f8f6f4 with cbsz:2
// blgp:2 (E2M3 x E2M3, one E8M0 scale per 32-wide k block of either operand).
// prep_mx6_kernel, the queries' side of the call, lives here too: it quantises
// by the rows' own device function (quantize_row_mx6, lmi_quant.hpp).
#include "lmi_quant.hpp"
#include "lmi_scan3.hpp"

#include <algorithm>
#include <mutex>
#include <utility>

namespace lmi {
namespace {

using i32x2 = int __attribute__((ext_vector_type(2)));
using i32x4 = int __attribute__((ext_vector_type(4)));
using i32x8 = int __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------------------
// Kept from the ring family (lmi_scan_ring_i8.hip, lmi_scan_ring_mx4.hip): the
// tile queue, the wave -> slot numbering, the early / late stagger of the two
// waves of a SIMD, the epilogue filter and the list walk, the partial layout
// with S = 1 and the bound exchange with its in-branch vmcnt(0) (the mx4 file
// says why).  Decided anew for 24-byte fragments:
//
//   operands : MFMA t covers k = 64 t + [0, 64).  Lane l holds the 24-byte
//              fragment (32 E2M3 codes, six of the operand's eight VGPRs) of
//              row / query l % 32 in k block 2 t + l / 32, and its scale
//              operand is the byte of exactly that (row, block): 12 MFMAs per
//              32-row block, as on mx4
//   per wave : 32 queries for the whole tile in 12 x 6 VGPRs of codes and 3
//              VGPRs of scale bytes (byte t & 3 of register t >> 2, picked by
//              op_sel): 75 registers (mx4: 51, i8: 96)
//   HBM      : a row is its 24 fragments back to back, 576 bytes; the scale
//              bytes lie behind the codes, even blocks first then odd blocks,
//              as on mx4 (lane half h reads three dwords at 12 h)
//   DMA      : 16-byte pieces.  Rows 4 w .. 4 w + 3 are 2304 consecutive bytes
//              of HBM and of LDS alike, 144 pieces: a straight copy by two
//              64-lane and one 16-lane buffer_load_dwordx4 ... lds (lane i of
//              instruction j: piece 64 j + i, which the hardware puts at 16 i
//              of the instruction's image; the images lie back to back).  576
//              = 36 x 16, so no piece straddles two rows and a row past the
//              chunk's end reads as zeros.  (The 12-byte LDS-DMA was tried
//              first: it puts lane i's piece at 16 i, not 12 i, leaving a hole
//              of four bytes a piece -- 24 KiB a block, and the ring would not
//              fit.)  With the wave's 96 scale bytes (24 lanes x 4 B) and 4
//              norms that is NDMA = 5 VM operations a block a wave, always:
//              the unit of the loop's vmcnt waits
//   LDS image: a wave's piece has the pitch PIECEP = 2304 + 8 bytes; the DMA
//              takes a destination that is 8-byte aligned (probed on the
//              hardware, and tests/test_gpu_mx6.py's exact case rests on it).
//              Fragment (row r = 4 w + x, block b) sits at
//                  w * 2312 + 576 x + 24 b
//              and is read as three ds_read_b64, each 8-byte aligned.  A
//              ds_read_b64 serves 32 lanes a pass (64 banks x 4 B = 32 slots
//              of 8 bytes); the lanes of a pass are one half h: same block,
//              same third of the fragment, rows r = 0 .. 31.  In units of 8
//              bytes the slot is
//                  289 w + 72 x + const  =  (w + 8 x + const) mod 32
//              since 289 = 9 * 32 + 1 and 72 = 2 * 32 + 8: x picks a multiple
//              of 8, w = 0 .. 7 the residue below it -- 32 rows on 32 distinct
//              slots, no conflict.  Without the 8-byte pad the pitch would be
//              288 = 0 mod 32 slots: eight-way.  A 24-byte stride is no power
//              of two, so the i8 / mx4 argument ((r + 4 c) mod 16 on 16-byte
//              slots) does not carry over; this one rests on the pitch being
//              1 mod 32 in 8-byte slots and a row being 8 mod 32 of them
//   ring     : four slots of one 32-row block (18 496 B with the pads), three
//              blocks in flight ahead of the one being multiplied, as on mx4.
//              A block costs mx4's matrix time (if FP6 runs at the FP4 rate)
//              and 1.45 x its bytes, so this kernel sits further to the
//              memory side than mx4 and wants at least mx4's cover: three
//              blocks are 55 KiB a CU in flight, the order of HBM's
//              bandwidth-delay product per CU (8 TB/s x 1.5-2 us / 256 CUs =
//              47-62 KB).  A fifth slot would still fit the 160 KiB at KL = 16
//              (162 176 B) but leave no room for anything else; it was not
//              tried.  143 680 B of LDS at KL = 16, 119 104 B at KL = 10
//   not here : tags, seeds, join workgroups, the tail split, nearest-chunk-
//              first, lower bounds, the wide / collect / band modes
// ---------------------------------------------------------------------------
namespace r6 {
constexpr int D = 768;
constexpr int FB = 24;                 // bytes of a fragment: 32 codes of 6 bits
constexpr int CB = D / 32 * FB;        // code bytes of a row (576)
constexpr int SB = D / 32;             // scale bytes of a row
constexpr int IMG = 64 * 16;           // LDS image of one full code DMA: 64 lanes x 16 B
constexpr int NPC = 4 * CB / 16;       // 16-byte pieces of a wave's four rows (144)
constexpr int NIMG = (NPC + 63) / 64;  // code DMAs of a wave per block (3: 64 + 64 + 16 lanes)
constexpr int PIECEP = 4 * CB + 8;     // a wave's piece: 1 mod 32 in 8-byte slots
constexpr int BLOCK = 8 * PIECEP;
constexpr int NSLOT = 4;               // ring slots (blocks)
constexpr int PF = 3;                  // blocks in flight ahead of the current one
constexpr int NDMA = NIMG + 2;         // VM operations of a wave per block
constexpr int SC_OFF = NSLOT * BLOCK;  // the slots' scale bytes, row-major [32][24]
constexpr int SCB = 32 * SB;
// the 32 norms of a block: read by the late waves one barrier after the
// block's codes, so a norm area lives one block longer than a code slot
constexpr int NNORM = 8;
constexpr int NORM_OFF = SC_OFF + NSLOT * SCB;
constexpr int LIST_OFF = NORM_OFF + NNORM * 128;
constexpr int NW = 8;
constexpr int QB = NW * 32;
constexpr int NQF = D / 64;            // MFMAs per block (and query fragments per lane)
// a query in qbuf: 576 code bytes, 24 scale bytes (the rows' order), 8 unused
constexpr int QPITCH = CB + 32;
template <int KL>
constexpr size_t kLds = (size_t)LIST_OFF + (size_t)NW * 64 * KL * 8 + 64;
static_assert(kLds<16> <= 160 * 1024, "LDS budget");
static_assert(QB == v3::QB, "the plan's tile width");
static_assert(PF < NSLOT && PF + 2 <= NNORM, "ring depth");
static_assert(CB % 16 == 0 && (PIECEP / 8) % 32 == 1 && (CB / 8) % 32 == 8 && PIECEP % 8 == 0, "the piece pitch");
static_assert(PF * NDMA < 64, "vmcnt is six bits");
}  // namespace r6

// a fragment as three aligned 8-byte words
struct Frag6 {
    i32x2 a, b, c;
};
__device__ __forceinline__ Frag6 frag6_load(const unsigned char* p) {
    const i32x2* w = reinterpret_cast<const i32x2*>(p);
    return Frag6{w[0], w[1], w[2]};
}
__device__ __forceinline__ i32x8 frag6_operand(const Frag6& f) {
    const i32x4 lo = __builtin_shufflevector(f.a, f.b, 0, 1, 2, 3);
    const i32x4 hi = __builtin_shufflevector(f.c, f.c, 0, 1, -1, -1);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, -1, -1);
}

// acc += A (rows) x B (queries) over k block pair T; the scale bytes of both
// operands are byte T & 3 of the registers given
template <int T>
__device__ __forceinline__ f32x16 mfma_mx6(const Frag6& af, const Frag6& qf, const f32x16& acc, int sa, int sq) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(frag6_operand(af), frag6_operand(qf), acc, 2, 2, T & 3, sa,
                                                           T & 3, sq);
}

template <int KL>
__global__ __launch_bounds__(512, 1) void scan3_mx6_kernel(ScanMx4Args ma) {
    static_assert(KL == 10 || KL == 16, "10- or 16-entry lists");
    using namespace r6;
    const Scan2Args& a = ma.s;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* ring = smem;
    // entry i of lane l of wave w at LIST_OFF + w * 512 KL + i * 512 + l * 8
    uint64_t* lists = reinterpret_cast<uint64_t*>(smem + LIST_OFF);
    int* wtab = reinterpret_cast<int*>(lists + NW * 64 * KL);  // [NW] SIMD ids, [NW] tile
    int& s_tile = wtab[NW];
    const unsigned char* corpus = reinterpret_cast<const unsigned char*>(a.corpus);
    const unsigned char* qbuf = reinterpret_cast<const unsigned char*>(a.qbuf);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ng = a.ng;

    // SIMD-balanced slot of this wave: order waves by (rank on their SIMD, SIMD)
    int simd, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID, 4, 2)" : "=s"(simd));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
    if (lane == 0) wtab[wave] = simd;
    __syncthreads();
    int slot = 0;
    {
        int key_me = simd;
        for (int w = 0; w < wave; ++w) key_me += (wtab[w] == simd) ? 4 : 0;  // + rank * 4
        for (int w = 0; w < NW; ++w) {
            int kw = wtab[w];
            for (int v = 0; v < w; ++v) kw += (wtab[v] == wtab[w]) ? 4 : 0;
            slot += (kw < key_me || (kw == key_me && w < wave)) ? 1 : 0;
        }
        slot = __builtin_amdgcn_readfirstlane(slot);
    }
    const int gx = xcc & (ng - 1);
    const bool late = slot >= NW / 2;
    const uint32_t lbase = (uint32_t)(uintptr_t)(lists + wave * 64 * KL) + (uint32_t)lane * 8u;  // this lane's list

    for (;;) {
        if (tid == 0) s_tile = dequeue_tile(a.meta, a.work, gx, ng);
        __syncthreads();
        const int t = __builtin_amdgcn_readfirstlane(s_tile);
        if (t < 0) break;
        const Tile tile = a.tiles[t];
        const int64_t row0 = a.bucket_off[tile.c] + (int64_t)tile.chunk * a.chunk_rows;
        const int nrows = __builtin_amdgcn_readfirstlane(
            (int)std::min<int64_t>(a.chunk_rows, a.bucket_off[tile.c + 1] - row0));
        const uint32_t r0lo = __builtin_amdgcn_readfirstlane((uint32_t)row0);
        const uint32_t r0hi = __builtin_amdgcn_readfirstlane((uint32_t)(row0 >> 32));
        const int64_t row0u = (int64_t)(((uint64_t)r0hi << 32) | r0lo);
        const int np = __builtin_amdgcn_readfirstlane(tile.np);
        const bool wave_live = 32 * slot < np;
        const int h = opaque(lane) >> 5;
        const int col = lane & 31;
        const bool live = 32 * slot + col < np;
        const int pp = tile.pp0 + 32 * slot + col;

        // the descriptors' sizes are the chunk's real bytes: rows past its end
        // read as zeros (scale bytes and norms too) and are masked by the row
        // count; a 16-byte piece lies inside one row, so it is whole or zero
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(corpus + row0u * CB), (short)0, nrows * CB, 0x00020000);
        const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(ma.scales + row0u * SB), (short)0, nrows * SB, 0x00020000);
        const __amdgpu_buffer_rsrc_t rn = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(a.inv_norm + row0u), (short)0, nrows * 4, 0x00020000);

        const int nblk = (nrows + 31) / 32;
        // This wave's share of block b, into ring slot b % NSLOT: rows 4 w ..
        // 4 w + 3 (lane i of code DMA j: piece 64 j + i of their 144, to 16 i
        // of image j; the third DMA has 16 lanes),
        // their 96 scale bytes and their 4 norms (area b % NNORM).  Always
        // NDMA wave instructions, whatever the lanes that take part.
        auto dma_block = [&](int b) {
            unsigned char* dst = ring + (b & (NSLOT - 1)) * BLOCK + wave * PIECEP;
            const int ln = opaque(lane);
            const uint32_t vo = (uint32_t)(4 * wave * CB + ln * 16);
#pragma unroll
            for (int j = 0; j < NIMG; ++j)
                if (64 * j + ln < NPC)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_t)(dst + j * IMG), 16, vo + j * IMG,
                                                             b * (32 * CB), 0, 0);
            if (ln < 24)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(
                    rc, (lds_t)(ring + SC_OFF + (b & (NSLOT - 1)) * SCB + wave * (4 * SB)), 4,
                    (uint32_t)(wave * (4 * SB) + ln * 4), b * SCB, 0, 0);
            if (ln < 4)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(
                    rn, (lds_t)(ring + NORM_OFF + (b & (NNORM - 1)) * 128 + 16 * wave), 4,
                    (uint32_t)((4 * wave + ln) * 4), b * 128, 0, 0);
        };
        // The first PF blocks' DMA goes out before the query fragments are
        // loaded (the ring is free: the previous tile drained it before its
        // closing barrier)
#pragma unroll
        for (int b = 0; b < PF; ++b)
            if (b < nblk) dma_block(b);

        Frag6 qf[NQF];
        int qs[3] = {0, 0, 0};
        // the lane's bound: only rows with ord(d) <= thr can enter the pair's
        // top-KL (a distance word: the bound may come from another chunk, so
        // ties at it survive to the chunk merge)
        uint32_t thr = 0u;
        float my_invq = 0.0f;
        int cnt = 0;  // entries in this lane's list; < KL: an unsorted append buffer
        if (wave_live) {
            const int q = live ? a.pair_q[pp] / a.R : 0;
            const unsigned char* qrow = qbuf + (size_t)q * QPITCH;
            // dead columns of a partial wave multiply zeros (scale byte 0 = 2^-127)
            const Frag6 z{};
#pragma unroll
            for (int s = 0; s < NQF; ++s) qf[s] = live ? frag6_load(qrow + FB * (2 * s + h)) : z;
#pragma unroll
            for (int s = 0; s < 3; ++s)
                qs[s] = live ? *reinterpret_cast<const int*>(qrow + CB + 12 * h + 4 * s) : 0;
            thr = live ? (uint32_t)(a.thr_g[pp] >> 32) : 0u;  // dead slots reject everything
            my_invq = live ? a.invq[q] : 0.0f;
        }
        {
            uint64_t E[KL];
            list_clear<KL>(E);
            list_store<KL>(opaque_u(lbase), E);
        }
        __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
        __syncthreads();

        // a lane's A-fragment base inside a block (row col, block h of a pair)
        const uint32_t lane_off = (uint32_t)((col >> 2) * PIECEP + (col & 3) * CB + h * FB);
        const uint32_t sc_off = (uint32_t)(SC_OFF + col * SB + h * 12);

        f32x16 acc{};
        uint32_t xg_carry = 0xffffffffu;  // global bound fetched, not yet applied
        // ---- epilogue of block eb (the sums of its 12 MFMAs in acc) ----------
        auto epilogue = [&](int eb) {
            const int ln = opaque(lane);
            const int hh = ln >> 5;
            const unsigned char* nb = ring + NORM_OFF + (eb & (NNORM - 1)) * 128 + hh * 16;
            const int vr = nrows - eb * 32 - 4 * hh;  // valid rows past this lane's offset
            thr = std::min(thr, xg_carry);
            xg_carry = 0xffffffffu;
            const float bound = key_dist_bound((uint64_t)thr << 32);
            const f32x16 accf = acc;
            // the filter: a candidate mask, one bit per register, register 0
            // in bit 15; only the chunk's last block checks the row count
            uint32_t mask = 0;
            auto filter = [&]<bool TAIL>() {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 n4 = *reinterpret_cast<const f32x4*>(nb + 32 * g);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float d = fmaf(-accf[4 * g + e], my_invq * n4[e], 1.0f);
                        bool ok = d <= bound;
                        if (TAIL) ok = ok && e + 8 * g < vr;
                        mask = mask + mask + (ok ? 1u : 0u);
                    }
                }
            };
            if (eb + 1 < nblk)
                filter.template operator()<false>();
            else
                filter.template operator()<true>();
            if (__any(mask != 0)) {
                const uint32_t rb = (uint32_t)(row0u + eb * 32 + 4 * hh);
                // every lane walks its own candidates, lowest register first
                // (rows ascending: a list ordered by distance with equal
                // distances in arrival order is ordered by key)
                uint32_t m = mask;
                const uint32_t la = opaque_u(lbase);
#pragma unroll 1
                while (__any(m != 0)) {
                    if (m != 0) {
                        const int hb = 31 - __builtin_clz(m);
                        m ^= 1u << hb;
                        const int rg = 15 - hb;
                        const int i = (rg & 3) + 8 * (rg >> 2);
                        const float n1 = *reinterpret_cast<const float*>(nb + i * 4);
                        const float d = fmaf(-select16(accf, rg), my_invq * n1, 1.0f);
                        const uint64_t key = make_key(d, rb + (uint32_t)i);
                        if (cnt < KL) {
                            // append mode: the first KL candidates are stored
                            // unsorted; a full buffer is sorted once (stable)
                            lds_put_u64(la + (uint32_t)cnt * 512u, key);
                            if (++cnt == KL) {
                                uint64_t L[KL];
                                list_load<KL>(la, L);
                                list_sort_hi<KL>(L);
                                list_store<KL>(la, L);
                                thr = std::min(thr, (uint32_t)(L[KL - 1] >> 32));
                            }
                        } else {
                            uint64_t L[KL];
                            list_load<KL>(la, L);
                            if ((uint32_t)(key >> 32) < (uint32_t)(L[KL - 1] >> 32)) {
                                list_insert_hi<KL>(L, key);
                                list_store<KL>(la, L);
                            }
                            thr = std::min(thr, (uint32_t)(L[KL - 1] >> 32));
                        }
                    }
                }
                // every bound is an upper bound of the pair's k-th key: share it
                thr = std::min(thr, partner_u32(thr, hh));
            }
        };
        // The two waves of a SIMD are staggered as in the other rings: the early
        // wave (slots 0-3) runs block b's MFMAs and then its epilogue; the late
        // wave (slots 4-7) runs block b-1's epilogue first (its sums carried
        // across the barrier) and then block b's MFMAs.
        const bool defer = late && wave_live;
        for (int blk = 0; blk < nblk; ++blk) {
            // one barrier per block: this wave's DMA of block blk has landed
            // (only the newer blocks', NDMA operations each, may still be in
            // flight; VM operations complete in order) and, past the barrier,
            // every wave's has, and every wave is done with block blk-1's slot
            const int ahead = std::min(PF - 1, nblk - 1 - blk);
            if (ahead >= 2)
                __builtin_amdgcn_s_waitcnt(waitcnt_vm(2 * NDMA));
            else if (ahead == 1)
                __builtin_amdgcn_s_waitcnt(waitcnt_vm(NDMA));
            else
                __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            // block blk+PF's DMA (its slot is block blk-1's, free past the
            // barrier; its norm area was block blk+PF-NNORM's): the early wave
            // ahead of its MFMAs, the late wave right after its deferred epilogue
            const bool more = blk + PF < nblk;
            if (more && !late) dma_block(blk + PF);
            if (defer && blk > 0) epilogue(blk - 1);
            if (more && late) dma_block(blk + PF);
            // every 32 blocks: publish this lane's bound to the pair's global
            // bound and take the global one back (tiles of the same pair on
            // other chunks run concurrently); consumed in the next epilogue.
            // The returning atomic is waited for here, inside its branch, as
            // in the mx4 ring (lmi_scan_ring_mx4.hip says why)
            if ((blk & 31) == 31 && live) {
                const uint32_t g = (uint32_t)(atomicMin(&a.thr_g[pp], ((unsigned long long)thr << 32) | 0xffffffffull) >> 32);
                __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
                xg_carry = std::min(xg_carry, g);
            }
            if (!wave_live) continue;
            {
                const unsigned char* rp = ring + (blk & (NSLOT - 1)) * BLOCK + opaque_u(lane_off);
                const int* sp = reinterpret_cast<const int*>(ring + (blk & (NSLOT - 1)) * SCB + opaque_u(sc_off));
                const int sa0 = sp[0], sa1 = sp[1], sa2 = sp[2];
                // MFMA tt: block 2 tt + h of the row, 48 tt past the lane's base
#define LMI_A6(tt) frag6_load(rp + (tt) * (2 * FB))
                Frag6 af[NQF];
#pragma unroll
                for (int tt = 0; tt < 3; ++tt) af[tt] = LMI_A6(tt);
                [&]<int... TT>(std::integer_sequence<int, TT...>) {
                    (([&] {
                         if (TT + 3 < NQF) af[(TT + 3) % NQF] = LMI_A6(TT + 3);
                         acc = mfma_mx6<TT>(af[TT], qf[TT], TT == 0 ? f32x16{} : acc,
                                            TT < 4 ? sa0 : TT < 8 ? sa1 : sa2, qs[TT >> 2]);
                         // keep the A-fragment reads 3 MFMAs ahead, no further
                         __builtin_amdgcn_sched_barrier(0);
                     }()),
                     ...);
                }(std::make_integer_sequence<int, NQF>{});
#undef LMI_A6
            }
            if (defer) continue;
            epilogue(blk);
        }
        if (defer && nblk > 0) epilogue(nblk - 1);
        // lanes still in append mode hold an unsorted (EMPTY-padded) buffer
        if (__any(cnt < KL)) {
            if (cnt < KL) {
                uint64_t L[KL];
                list_load<KL>(lbase, L);
                list_sort<KL>(L);
                list_store<KL>(lbase, L);
            }
        }
        __syncthreads();  // every wave's DMA drained (the tail waited vmcnt(0))

        // ---- merge the two partial lists of each query (lanes col, col+32) ----
        if (h == 0 && live) {
            uint64_t L[KL], P[KL];
            list_load<KL, 0>(lbase, L);
            list_load<KL, 32 * 8>(lbase, P);
#pragma unroll
            for (int i = 0; i < KL; ++i) {
                if (P[i] >= L[KL - 1]) break;
                list_insert<KL>(L, P[i]);
            }
            uint64_t* out = a.partial + ((size_t)pp * a.max_chunks + tile.chunk) * KL;
#pragma unroll
            for (int i = 0; i < KL; ++i) out[i] = L[i];
            if (L[KL - 1] != kEmptyKey) atomicMin(&a.thr_g[pp], (unsigned long long)L[KL - 1]);
        }
    }
}

// prep_kernel for an LMI_MX6 scan: qbuf = every query's MXFP6 fragments and
// scale bytes ([nq] records of r6::QPITCH bytes) and invq = the codes' 1/n, by
// the rows' own device function; the output prefill and the call's word fills
template <bool VEC>
__global__ __launch_bounds__(kThreads) void prep_mx6_kernel(const float* __restrict__ q, int32_t nq, int32_t ldq,
                                                            int32_t d, int32_t d_pad, uint8_t* __restrict__ qbuf,
                                                            float* __restrict__ invq, float* __restrict__ out_d,
                                                            int32_t* __restrict__ out_pos,
                                                            int32_t* __restrict__ out_row, int32_t out_per_q,
                                                            WordFills fills) {
    const int row = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= nq) return;  // (wave-uniform; no block-wide barrier below)
    uint8_t* rec = qbuf + (size_t)row * r6::QPITCH;
    const float inv = quantize_row_mx6<float, VEC>(q + (size_t)row * ldq, d, d_pad, lane, rec, rec + r6::CB);
    if (lane == 0) invq[row] = inv;
    for (int e = lane; e < out_per_q; e += 64) {
        out_d[(size_t)row * out_per_q + e] = __builtin_inff();
        out_pos[(size_t)row * out_per_q + e] = -1;
        if (out_row) out_row[(size_t)row * out_per_q + e] = -1;
    }
    for (int f = 0; f < fills.n; ++f)
        for (int e = lane; e < fills.per_q[f]; e += 64)
            fills.p[f][(size_t)row * fills.per_q[f] + e] = fills.v[f];
}

}  // namespace

size_t mx6_qbuf_bytes(int nq) { return (size_t)nq * r6::QPITCH; }

int launch_prep_mx6(const float* q, int32_t nq, int32_t ldq, int32_t d, int32_t d_pad, void* qbuf, float* invq,
                    float* out_d, int32_t* out_pos, int32_t* out_row, int32_t out_per_q, const WordFills& fills,
                    hipStream_t s) {
    if (d_pad != r6::D) {
        set_error("LMI_MX6: d_pad=%d (the 6-bit storage takes d_pad == %d)", d_pad, r6::D);
        return LMI_E_INVALID;
    }
    const dim3 pg((nq + kThreads / 64 - 1) / (kThreads / 64));
    const bool vec = ((uintptr_t)q % 16 == 0) && (ldq % 4 == 0);
    hipLaunchKernelGGL(vec ? prep_mx6_kernel<true> : prep_mx6_kernel<false>, pg, dim3(kThreads), 0, s, q, nq, ldq, d,
                       d_pad, static_cast<uint8_t*>(qbuf), invq, out_d, out_pos, out_row, out_per_q, fills);
    LMI_LAUNCH_CHECK("prep_mx6_kernel");
    return LMI_OK;
}

// one launch of the persistent grid (one workgroup per CU, dynamic LDS); HIP
// events around it while lmi_timing_enable is on
template <int KL>
int launch_scan3_mx6(const ScanMx4Args& b, hipStream_t s) {
    static std::once_flag once;
    static hipError_t attr_err = hipSuccess;
    std::call_once(once, [] {
        attr_err = hipFuncSetAttribute((const void*)scan3_mx6_kernel<KL>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)r6::kLds<KL>);
    });
    LMI_HIP_TRY(attr_err);
    const bool timed = timing().on;
    std::pair<hipEvent_t, hipEvent_t> ev{};
    if (timed) {
        const int rc = timing_record(s, true, ev);
        if (rc != LMI_OK) return rc;
    }
    hipLaunchKernelGGL((scan3_mx6_kernel<KL>), dim3(scan_grid()), dim3(r6::NW * 64), r6::kLds<KL>, s, b);
    LMI_LAUNCH_CHECK("scan3_mx6_kernel");
    if (timed) return timing_record(s, false, ev);
    return LMI_OK;
}

template int launch_scan3_mx6<10>(const ScanMx4Args&, hipStream_t);
template int launch_scan3_mx6<16>(const ScanMx4Args&, hipStream_t);

}  // namespace lmi
