// scan3_mx4_kernel / scan3_mx6_kernel: the 8-wave ring on the MXFP4 codes of
// the 4-bit storage (LMI_MX4 / LMI_Q_MX4) and on the MXFP6 codes of the 6-bit
// storage (LMI_MX6 / LMI_Q_MX6; include/lmi_hip.h "the MXFP4 format", "the
// MXFP6 format"), d_pad == 768, plain lists of 10 or 16 entries.  The families
// ScanKernel::Ring8MX4 / Ring8MX6 of the scan's plan.  Products run on
// v_mfma_scale_f32_32x32x64_f8f6f4 with cbsz:4 blgp:4 (E2M1 x E2M1) or cbsz:2
// blgp:2 (E2M3 x E2M3), one E8M0 scale per 32-wide k block of either operand.
// One body, ring_mx_body, over a format's traits (Mx4, Mx6); the two kernels
// are its instances under their own names.  prep_mx4_kernel / prep_mx6_kernel,
// the queries' side of the call, live here too: they quantise by the rows' own
// device functions (quantize_row_mx4 / _mx6, lmi_quant.hpp).
#include "lmi_quant.hpp"
#include "lmi_ring8.hpp"

namespace lmi {
namespace {

using i32x2 = int __attribute__((ext_vector_type(2)));
using i32x4 = int __attribute__((ext_vector_type(4)));
using i32x8 = int __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------------------
// The i8 ring's structure (lmi_scan_ring_i8.hip: tile queue, wave -> slot
// numbering, staggered waves of a SIMD, epilogue, list walk; the list clear and
// the tile end with its partial layout are lmi_ring8.hpp's) with these
// differences in both formats:
//
//   operands : one MFMA covers k = 64 t + [0, 64).  Lane l holds the fragment
//              (32 codes) of row / query l % 32 in k block 2 t + l / 32, and
//              its scale operand is the byte of exactly that (row, block): 12
//              MFMAs per 32-row block
//   per wave : 32 queries for the whole tile in 12 fragments of codes and 3
//              VGPRs of scale bytes (byte t & 3 of register t >> 2, picked by
//              op_sel)
//   scales   : a row's 24 bytes are stored even blocks first, then odd blocks
//              (quantize_row_mx4 / _mx6), so lane half h reads the 12 bytes of
//              its MFMAs as three dwords at 12 h: no byte shuffles in the loop
//   ring     : four slots of one 32-row block and the block's 768 scale bytes,
//              three blocks in flight ahead of the one being multiplied (the
//              i8 ring: one).  A block is cheaper on the matrix pipe than its
//              bytes are on HBM, so the freed LDS goes to latency cover, not
//              to a second workgroup
//   DMA      : wave w brings rows 4 w .. 4 w + 3 of a block whole: their codes
//              (the format's dma_codes), their 96 scale bytes (24 lanes x 4 B)
//              and 4 norms: NDMA VM operations a block, always, the unit of
//              the loop's vmcnt waits
//   not here : tags, seeds, join workgroups, the tail split, nearest-chunk-
//              first, lower bounds, the wide / collect / band modes
// ---------------------------------------------------------------------------
// The LDS layout of a format with CB code bytes a row, a wave's piece (its four
// rows) padded by PAD bytes and NDMA VM operations of a wave per block
template <int CB_, int PAD, int NDMA_>
struct MxLayout {
    static constexpr int D = 768;
    static constexpr int CB = CB_;               // code bytes of a row
    static constexpr int SB = D / 32;            // scale bytes of a row
    static constexpr int PIECEP = 4 * CB + PAD;  // piece pitch
    static constexpr int BLOCK = 8 * PIECEP;
    static constexpr int NSLOT = 4;              // ring slots (blocks)
    static constexpr int PF = 3;                 // blocks in flight ahead of the current one
    static constexpr int NDMA = NDMA_;
    static constexpr int SC_OFF = NSLOT * BLOCK;  // the slots' scale bytes, row-major [32][24]
    static constexpr int SCB = 32 * SB;
    // the 32 norms of a block: read by the late waves one barrier after the
    // block's codes, so a norm area lives one block longer than a code slot
    static constexpr int NNORM = 8;
    static constexpr int NORM_OFF = SC_OFF + NSLOT * SCB;
    static constexpr int LIST_OFF = NORM_OFF + NNORM * 128;
    static constexpr int NW = 8;
    static constexpr int QB = NW * 32;
    static constexpr int NQF = D / 64;           // MFMAs per block (and query fragments per lane)
    // a query in qbuf: CB code bytes, 24 scale bytes (the rows' order), 8 unused
    static constexpr int QPITCH = CB + 32;
    // mx4: 96 320 bytes for KL = 10, 120 896 for KL = 16; mx6: 119 104, 143 680
    template <int KL>
    static constexpr size_t kLds = (size_t)LIST_OFF + (size_t)NW * 64 * KL * 8 + 64;
    static_assert(kLds<16> <= 160 * 1024, "LDS budget");
    static_assert(QB == v3::QB, "the plan's tile width");
    static_assert(PF < NSLOT && PF + 2 <= NNORM, "ring depth");
    static_assert(PF * NDMA < 64, "vmcnt is six bits");
};

// MXFP4: a fragment is 16 bytes, four VGPRs (12 x 4 + 3 = 51 registers of
// queries where the i8 ring holds 96); a block is 12.5 KiB with the pads.
// LDS image of a wave's piece: its four rows interleaved at 16-B granularity
// (row 4p + x, chunk c of the row at 64 c + 16 x), pieces at a 1600-B pitch.
// Row r chunk c sits at (r >> 2) * 1600 + 16 (r & 3) + 64 c; its 16-B bank
// slot is (100 (r >> 2) + (r & 3) + 4 c) mod 16 = (r + 4 c) mod 16.  Every
// lane of a half reads the same c, and each 16-lane group of ds_read_b128
// holds 16 rows that differ mod 16 (lmi_scan_ring_i8.hip): no conflict.
// Without the 64-B pad the slot would be (r & 3) + 4 c: four-way.
struct Mx4 : MxLayout<768 / 2, 64, 4> {
    static constexpr const char* NAME = "LMI_MX4";
    static constexpr int BITS = 4;
    using Frag = i32x4;
    static constexpr int A_STEP = 128;  // MFMA tt: chunk 2 tt + h of the row, 128 tt past the lane's base
    static __device__ __forceinline__ Frag load_frag(const unsigned char* p) {
        return *reinterpret_cast<const i32x4*>(p);
    }
    // query fragment s of lane half h in a qbuf record
    static __device__ __forceinline__ int q_off(int s, int h) { return 32 * s + 16 * h; }
    // a lane's A-fragment base inside a block (row col, chunk h of a pair)
    static __device__ __forceinline__ uint32_t lane_off(int col, int h) {
        return (uint32_t)((col >> 2) * PIECEP + (col & 3) * 16 + h * 64);
    }
    // acc += A (rows) x B (queries) over k block pair T; the scale bytes of both
    // operands are byte T & 3 of the registers given
    template <int T>
    static __device__ __forceinline__ f32x16 mfma(const Frag& af, const Frag& qf, const f32x16& acc, int sa, int sq) {
        const i32x8 a8 = __builtin_shufflevector(af, af, 0, 1, 2, 3, -1, -1, -1, -1);
        const i32x8 q8 = __builtin_shufflevector(qf, qf, 0, 1, 2, 3, -1, -1, -1, -1);
        return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, q8, acc, 4, 4, T & 3, sa, T & 3, sq);
    }
    // the codes of rows 4 w .. 4 w + 3 of block b: 96 16-byte chunks, one
    // 64-lane and one 32-lane DMA (lane l of the first: row 4 w + (l & 3),
    // chunk l >> 2, to LDS slot l of the piece; the second: chunks 16 .. 23)
    static __device__ __forceinline__ void dma_codes(__amdgpu_buffer_rsrc_t rs, unsigned char* dst, int wave, int ln,
                                                     int b) {
        const uint32_t vo = (uint32_t)((4 * wave + (ln & 3)) * CB + (ln >> 2) * 16);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_t)dst, 16, vo, b * (32 * CB), 0, 0);
        if (ln < 32)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_t)(dst + 1024), 16, vo + 256, b * (32 * CB), 0, 0);
    }
    template <bool VEC>
    static __device__ __forceinline__ float quantize(const float* src, int d, int d_pad, int lane, uint8_t* codes,
                                                     uint8_t* scales) {
        return quantize_row_mx4<float, VEC>(src, d, d_pad, lane, codes, scales);
    }
};

// MXFP6, decided anew for 24-byte fragments:
//
//   operands : lane l holds the 24-byte fragment (32 E2M3 codes, six of the
//              operand's eight VGPRs): 12 x 6 + 3 = 75 registers of queries
//              (mx4: 51, i8: 96)
//   HBM      : a row is its 24 fragments back to back, 576 bytes; the scale
//              bytes lie behind the codes, even blocks first then odd blocks,
//              as on mx4
//   DMA      : 16-byte pieces.  Rows 4 w .. 4 w + 3 are 2304 consecutive bytes
//              of HBM and of LDS alike, 144 pieces: a straight copy by two
//              64-lane and one 16-lane buffer_load_dwordx4 ... lds (lane i of
//              instruction j: piece 64 j + i, which the hardware puts at 16 i
//              of the instruction's image; the images lie back to back).  576
//              = 36 x 16, so no piece straddles two rows and a row past the
//              chunk's end reads as zeros.  (The 12-byte LDS-DMA was tried
//              first: it puts lane i's piece at 16 i, not 12 i, leaving a hole
//              of four bytes a piece -- 24 KiB a block, and the ring would not
//              fit.)  With the scale bytes and the norms NDMA = 5
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
//   ring     : a block is 18 496 B with the pads.  It costs mx4's matrix time
//              (if FP6 runs at the FP4 rate) and 1.45 x its bytes, so this
//              kernel sits further to the memory side than mx4 and wants at
//              least mx4's cover: three blocks are 55 KiB a CU in flight, the
//              order of HBM's bandwidth-delay product per CU (8 TB/s x 1.5-2
//              us / 256 CUs = 47-62 KB).  A fifth slot would still fit the 160
//              KiB at KL = 16 (162 176 B) but leave no room for anything else;
//              it was not tried
struct Mx6 : MxLayout<768 / 32 * 24, 8, 5> {
    static constexpr const char* NAME = "LMI_MX6";
    static constexpr int BITS = 6;
    static constexpr int FB = 24;                 // bytes of a fragment: 32 codes of 6 bits
    static constexpr int IMG = 64 * 16;           // LDS image of one full code DMA: 64 lanes x 16 B
    static constexpr int NPC = 4 * CB / 16;       // 16-byte pieces of a wave's four rows (144)
    static constexpr int NIMG = (NPC + 63) / 64;  // code DMAs of a wave per block (3: 64 + 64 + 16 lanes)
    static_assert(CB == D / 32 * FB && NDMA == NIMG + 2, "VM operations of a wave per block");
    static_assert(CB % 16 == 0 && (PIECEP / 8) % 32 == 1 && (CB / 8) % 32 == 8 && PIECEP % 8 == 0, "the piece pitch");
    // a fragment as three aligned 8-byte words
    struct Frag {
        i32x2 a, b, c;
    };
    static constexpr int A_STEP = 2 * FB;  // MFMA tt: block 2 tt + h of the row, 48 tt past the lane's base
    static __device__ __forceinline__ Frag load_frag(const unsigned char* p) {
        const i32x2* w = reinterpret_cast<const i32x2*>(p);
        return Frag{w[0], w[1], w[2]};
    }
    static __device__ __forceinline__ i32x8 operand(const Frag& f) {
        const i32x4 lo = __builtin_shufflevector(f.a, f.b, 0, 1, 2, 3);
        const i32x4 hi = __builtin_shufflevector(f.c, f.c, 0, 1, -1, -1);
        return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, -1, -1);
    }
    static __device__ __forceinline__ int q_off(int s, int h) { return FB * (2 * s + h); }
    // a lane's A-fragment base inside a block (row col, block h of a pair)
    static __device__ __forceinline__ uint32_t lane_off(int col, int h) {
        return (uint32_t)((col >> 2) * PIECEP + (col & 3) * CB + h * FB);
    }
    template <int T>
    static __device__ __forceinline__ f32x16 mfma(const Frag& af, const Frag& qf, const f32x16& acc, int sa, int sq) {
        return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(operand(af), operand(qf), acc, 2, 2, T & 3, sa, T & 3,
                                                               sq);
    }
    // lane i of code DMA j: piece 64 j + i of the wave's 144, to 16 i of image
    // j (the third DMA has 16 lanes); a piece lies inside one row, so past the
    // chunk's end it is whole or zero
    static __device__ __forceinline__ void dma_codes(__amdgpu_buffer_rsrc_t rs, unsigned char* dst, int wave, int ln,
                                                     int b) {
        const uint32_t vo = (uint32_t)(4 * wave * CB + ln * 16);
#pragma unroll
        for (int j = 0; j < NIMG; ++j)
            if (64 * j + ln < NPC)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_t)(dst + j * IMG), 16, vo + j * IMG, b * (32 * CB),
                                                         0, 0);
    }
    template <bool VEC>
    static __device__ __forceinline__ float quantize(const float* src, int d, int d_pad, int lane, uint8_t* codes,
                                                     uint8_t* scales) {
        return quantize_row_mx6<float, VEC>(src, d, d_pad, lane, codes, scales);
    }
};

template <class F, int KL>
__device__ __forceinline__ void ring_mx_body(const ScanMx4Args& ma) {
    static_assert(KL == 10 || KL == 16, "10- or 16-entry lists");
    using Frag = typename F::Frag;
    constexpr int NSLOT = F::NSLOT, NNORM = F::NNORM, PF = F::PF, NDMA = F::NDMA, NQF = F::NQF, SB = F::SB;
    const Scan2Args& a = ma.s;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* ring = smem;
    // entry i of lane l of wave w at LIST_OFF + w * 512 KL + i * 512 + l * 8
    uint64_t* lists = reinterpret_cast<uint64_t*>(smem + F::LIST_OFF);
    int* wtab = reinterpret_cast<int*>(lists + F::NW * 64 * KL);  // [NW] SIMD ids, [NW] tile
    int& s_tile = wtab[F::NW];
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
        for (int w = 0; w < F::NW; ++w) {
            int kw = wtab[w];
            for (int v = 0; v < w; ++v) kw += (wtab[v] == wtab[w]) ? 4 : 0;
            slot += (kw < key_me || (kw == key_me && w < wave)) ? 1 : 0;
        }
        slot = __builtin_amdgcn_readfirstlane(slot);
    }
    const int gx = xcc & (ng - 1);
    const bool late = slot >= F::NW / 2;
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
        const int nblk = (nrows + 31) / 32;

        // the descriptors' sizes are the chunk's real bytes: rows past its end
        // read as zeros (scale bytes and norms too) and are masked by the row count
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(corpus + row0u * F::CB), (short)0, nrows * F::CB, 0x00020000);
        const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(ma.scales + row0u * SB), (short)0, nrows * SB, 0x00020000);
        const __amdgpu_buffer_rsrc_t rn = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(a.inv_norm + row0u), (short)0, nrows * 4, 0x00020000);

        // This wave's share of block b, into ring slot b % NSLOT: the codes of
        // rows 4 w .. 4 w + 3, their 96 scale bytes and their 4 norms (area b %
        // NNORM).  Always NDMA wave instructions, whatever the lanes that take part.
        auto dma_block = [&](int b) {
            unsigned char* dst = ring + (b & (NSLOT - 1)) * F::BLOCK + wave * F::PIECEP;
            const int ln = opaque(lane);
            F::dma_codes(rs, dst, wave, ln, b);
            if (ln < 24)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(
                    rc, (lds_t)(ring + F::SC_OFF + (b & (NSLOT - 1)) * F::SCB + wave * (4 * SB)), 4,
                    (uint32_t)(wave * (4 * SB) + ln * 4), b * F::SCB, 0, 0);
            if (ln < 4)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(
                    rn, (lds_t)(ring + F::NORM_OFF + (b & (NNORM - 1)) * 128 + 16 * wave), 4,
                    (uint32_t)((4 * wave + ln) * 4), b * 128, 0, 0);
        };
        // The first PF blocks' DMA goes out before the query fragments are
        // loaded (the ring is free: the previous tile drained it before its
        // closing barrier)
#pragma unroll
        for (int b = 0; b < PF; ++b)
            if (b < nblk) dma_block(b);

        Frag qf[NQF];
        int qs[3] = {0, 0, 0};
        // the lane's bound: only rows with ord(d) <= thr can enter the pair's
        // top-KL (a distance word: the bound may come from another chunk, so
        // ties at it survive to the chunk merge)
        uint32_t thr = 0u;
        float my_invq = 0.0f;
        int cnt = 0;  // entries in this lane's list; < KL: an unsorted append buffer
        if (wave_live) {
            const int q = live ? a.pair_q[pp] / a.R : 0;
            const unsigned char* qrow = qbuf + (size_t)q * F::QPITCH;
            // dead columns of a partial wave multiply zeros (scale byte 0 = 2^-127)
            const Frag z{};
#pragma unroll
            for (int s = 0; s < NQF; ++s) qf[s] = live ? F::load_frag(qrow + F::q_off(s, h)) : z;
#pragma unroll
            for (int s = 0; s < 3; ++s)
                qs[s] = live ? *reinterpret_cast<const int*>(qrow + F::CB + 12 * h + 4 * s) : 0;
            thr = live ? (uint32_t)(a.thr_g[pp] >> 32) : 0u;  // dead slots reject everything
            my_invq = live ? a.invq[q] : 0.0f;
        }
        ring_lists_clear<KL>(lbase);

        const uint32_t lane_off = F::lane_off(col, h);
        const uint32_t sc_off = (uint32_t)(F::SC_OFF + col * SB + h * 12);

        f32x16 acc{};
        uint32_t xg_carry = 0xffffffffu;  // global bound fetched, not yet applied
        // ---- epilogue of block eb (the sums of its 12 MFMAs in acc) ----------
        auto epilogue = [&](int eb) {
            const int ln = opaque(lane);
            const int hh = ln >> 5;
            const unsigned char* nb = ring + F::NORM_OFF + (eb & (NNORM - 1)) * 128 + hh * 16;
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
            // The returning atomic is waited for here, inside its branch
            // (once in 32 blocks the ring drains): left pending, its return
            // registers would make the compiler guard every reuse of them in
            // the loop with a vmcnt(0), and the ring would drain every block
            if ((blk & 31) == 31 && live) {
                const uint32_t g = (uint32_t)(atomicMin(&a.thr_g[pp], ((unsigned long long)thr << 32) | 0xffffffffull) >> 32);
                __builtin_amdgcn_s_waitcnt(waitcnt_vm(0));
                xg_carry = std::min(xg_carry, g);
            }
            if (!wave_live) continue;
            {
                const unsigned char* rp = ring + (blk & (NSLOT - 1)) * F::BLOCK + opaque_u(lane_off);
                const int* sp = reinterpret_cast<const int*>(ring + (blk & (NSLOT - 1)) * F::SCB + opaque_u(sc_off));
                const int sa0 = sp[0], sa1 = sp[1], sa2 = sp[2];
#define LMI_AMX(tt) F::load_frag(rp + (tt) * F::A_STEP)
                Frag af[NQF];
#pragma unroll
                for (int tt = 0; tt < 3; ++tt) af[tt] = LMI_AMX(tt);
                [&]<int... TT>(std::integer_sequence<int, TT...>) {
                    (([&] {
                         if (TT + 3 < NQF) af[(TT + 3) % NQF] = LMI_AMX(TT + 3);
                         acc = F::template mfma<TT>(af[TT], qf[TT], TT == 0 ? f32x16{} : acc,
                                                    TT < 4 ? sa0 : TT < 8 ? sa1 : sa2, qs[TT >> 2]);
                         // keep the A-fragment reads 3 MFMAs ahead, no further
                         __builtin_amdgcn_sched_barrier(0);
                     }()),
                     ...);
                }(std::make_integer_sequence<int, NQF>{});
#undef LMI_AMX
            }
            if (defer) continue;
            epilogue(blk);
        }
        if (defer && nblk > 0) epilogue(nblk - 1);
        ring_finish<KL>(a.partial, a.max_chunks, a.thr_g, pp, tile.chunk, h, live, lbase, cnt);
    }
}

template <int KL>
__global__ __launch_bounds__(512, 1) void scan3_mx4_kernel(ScanMx4Args ma) {
    ring_mx_body<Mx4, KL>(ma);
}
template <int KL>
__global__ __launch_bounds__(512, 1) void scan3_mx6_kernel(ScanMx4Args ma) {
    ring_mx_body<Mx6, KL>(ma);
}

// prep_kernel for an LMI_MX4 / LMI_MX6 scan: qbuf = every query's codes and
// scale bytes ([nq] records of QPITCH bytes) and invq = the codes' 1/n, by the
// rows' own device function; the output prefill and the call's word fills
template <class F, bool VEC>
__device__ __forceinline__ void prep_mx_body(const float* __restrict__ q, int32_t nq, int32_t ldq, int32_t d,
                                             int32_t d_pad, uint8_t* __restrict__ qbuf, float* __restrict__ invq,
                                             float* __restrict__ out_d, int32_t* __restrict__ out_pos,
                                             int32_t* __restrict__ out_row, int32_t out_per_q,
                                             const WordFills& fills) {
    const int row = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= nq) return;  // (wave-uniform; no block-wide barrier below)
    uint8_t* rec = qbuf + (size_t)row * F::QPITCH;
    const float inv = F::template quantize<VEC>(q + (size_t)row * ldq, d, d_pad, lane, rec, rec + F::CB);
    if (lane == 0) invq[row] = inv;
    prep_fill_tail(row, lane, out_d, out_pos, out_row, out_per_q, fills);
}
template <bool VEC>
__global__ __launch_bounds__(kThreads) void prep_mx4_kernel(const float* __restrict__ q, int32_t nq, int32_t ldq,
                                                            int32_t d, int32_t d_pad, uint8_t* __restrict__ qbuf,
                                                            float* __restrict__ invq, float* __restrict__ out_d,
                                                            int32_t* __restrict__ out_pos,
                                                            int32_t* __restrict__ out_row, int32_t out_per_q,
                                                            WordFills fills) {
    prep_mx_body<Mx4, VEC>(q, nq, ldq, d, d_pad, qbuf, invq, out_d, out_pos, out_row, out_per_q, fills);
}
template <bool VEC>
__global__ __launch_bounds__(kThreads) void prep_mx6_kernel(const float* __restrict__ q, int32_t nq, int32_t ldq,
                                                            int32_t d, int32_t d_pad, uint8_t* __restrict__ qbuf,
                                                            float* __restrict__ invq, float* __restrict__ out_d,
                                                            int32_t* __restrict__ out_pos,
                                                            int32_t* __restrict__ out_row, int32_t out_per_q,
                                                            WordFills fills) {
    prep_mx_body<Mx6, VEC>(q, nq, ldq, d, d_pad, qbuf, invq, out_d, out_pos, out_row, out_per_q, fills);
}

// the launch of a format's prep kernel (Vec: float4 loads of the query rows,
// 16-byte aligned and ldq % 4 == 0; Any: the other form)
template <class F, auto Vec, auto Any>
int launch_prep_mx(const char* kernel, const float* q, int32_t nq, int32_t ldq, int32_t d, int32_t d_pad, void* qbuf,
                   float* invq, float* out_d, int32_t* out_pos, int32_t* out_row, int32_t out_per_q,
                   const WordFills& fills, hipStream_t s) {
    if (d_pad != F::D) {
        set_error("%s: d_pad=%d (the %d-bit storage takes d_pad == %d)", F::NAME, d_pad, F::BITS, F::D);
        return LMI_E_INVALID;
    }
    const dim3 pg((nq + kThreads / 64 - 1) / (kThreads / 64));
    const bool vec = ((uintptr_t)q % 16 == 0) && (ldq % 4 == 0);
    hipLaunchKernelGGL(vec ? Vec : Any, pg, dim3(kThreads), 0, s, q, nq, ldq, d, d_pad, static_cast<uint8_t*>(qbuf),
                       invq, out_d, out_pos, out_row, out_per_q, fills);
    LMI_LAUNCH_CHECK(kernel);
    return LMI_OK;
}

// one launch of the persistent grid (one workgroup per CU, dynamic LDS)
template <class F, auto Kernel, int KL>
int launch_scan3_mx(const char* kernel, const ScanMx4Args& b, hipStream_t s) {
    return launch_dyn_lds<Kernel, (int)F::template kLds<KL>>(kernel, dim3(scan_grid()), dim3(F::NW * 64),
                                                             F::template kLds<KL>, s, b);
}

}  // namespace

size_t mx4_qbuf_bytes(int nq) { return (size_t)nq * Mx4::QPITCH; }
size_t mx6_qbuf_bytes(int nq) { return (size_t)nq * Mx6::QPITCH; }

int launch_prep_mx4(const float* q, int32_t nq, int32_t ldq, int32_t d, int32_t d_pad, void* qbuf, float* invq,
                    float* out_d, int32_t* out_pos, int32_t* out_row, int32_t out_per_q, const WordFills& fills,
                    hipStream_t s) {
    return launch_prep_mx<Mx4, prep_mx4_kernel<true>, prep_mx4_kernel<false>>(
        "prep_mx4_kernel", q, nq, ldq, d, d_pad, qbuf, invq, out_d, out_pos, out_row, out_per_q, fills, s);
}
int launch_prep_mx6(const float* q, int32_t nq, int32_t ldq, int32_t d, int32_t d_pad, void* qbuf, float* invq,
                    float* out_d, int32_t* out_pos, int32_t* out_row, int32_t out_per_q, const WordFills& fills,
                    hipStream_t s) {
    return launch_prep_mx<Mx6, prep_mx6_kernel<true>, prep_mx6_kernel<false>>(
        "prep_mx6_kernel", q, nq, ldq, d, d_pad, qbuf, invq, out_d, out_pos, out_row, out_per_q, fills, s);
}

template <int KL>
int launch_scan3_mx4(const ScanMx4Args& b, hipStream_t s) {
    return launch_scan3_mx<Mx4, scan3_mx4_kernel<KL>, KL>("scan3_mx4_kernel", b, s);
}
template <int KL>
int launch_scan3_mx6(const ScanMx4Args& b, hipStream_t s) {
    return launch_scan3_mx<Mx6, scan3_mx6_kernel<KL>, KL>("scan3_mx6_kernel", b, s);
}

template int launch_scan3_mx4<10>(const ScanMx4Args&, hipStream_t);
template int launch_scan3_mx4<16>(const ScanMx4Args&, hipStream_t);
template int launch_scan3_mx6<10>(const ScanMx4Args&, hipStream_t);
template int launch_scan3_mx6<16>(const ScanMx4Args&, hipStream_t);

}  // namespace lmi
