// bf16x3 variant of scan_mainloop.inc (same contract: textually included inside scan_xattn_kernel, leaves the raw
// 144 x 64 block parked transposed in sm.arawt).  Operands are the SPLIT planes of the fp32 inputs, x = hi + lo + O(2^-17 |x|)
// (scan_split_rows_kernel: per row and 32-wide K chunk the 64 B of hi are followed by the 64 B of lo, so one chunk of one row is
// ONE 128-byte line exactly like the fp32 operand -- with whole-row planes every load used half a line and the vector L1
// path (64 B/clk) became the limiter), and
// every dot product is  hi.hi + hi.lo + lo.hi  on v_mfma_f32_16x16x32_bf16 with fp32 accumulation: 27 MFMAs of 16 cycles per
// wave and 32-wide K chunk instead of 72 of 32 cycles -- 5.3x less matrix-pipe time, the same LDS and global traffic
// (two 2-byte planes = one 4-byte operand).  The C/D layout of the 16x16x32 bf16 MFMA equals the fp32 16x16x4 one, so the
// epilogue is shared unchanged.
// PREC bit 1 ("fp16x3"): the planes are fp16 instead of bf16 -- 11 + 11 mantissa bits, x = hi + lo + O(2^-22 |x|), essentially the
// whole fp32 mantissa.  The matrix core FLUSHES fp16 subnormals (measured: 1e-5 outliers in the scores without the scaling),
// so the operands are split as x' = 2^12 x and lo is stored scaled by another 2^11; the cross terms hi.lo' + lo'.hi accumulate in
// a SECOND accumulator set, and the park folds everything back with exact powers of two.  Needs |x| <= 15.99 (the operands of
// this path are unit-norm rows); v_mfma_f32_16x16x32_f16 runs at the bf16 rate.
//   LDS chunk layout: [plane][row][4 granules of 16 B = 8 bf16]; granule g of row r is stored at g ^ ((0 - (r >> 2)) & 3), and the
//   rows of plane 1 (lo) are stored at r ^ 1.  Round 5 (PMC r04: 47 % of the LDS cycles of this kernel were bank conflicts): a
//   ds_read_b128 is NOT serviced in the four quarter-waves but in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... (guide,
//   LDS): every group holds the 16 rows fi = 0..15 once, rows 0-3 / 12-15 from one k group and rows 4-11 from its neighbour (g ^ 1).
//   The four rows fi = q, q + 4, q + 8, q + 12 share the 64-byte quarter of the 256-byte bank window, so their granule slots
//   {g ^ p0, g ^ 1 ^ p1, g ^ 1 ^ p2, g ^ p3} must differ: p = (0, 3, 2, 1) does it (the round-3 map p = (0, 1, 2, 3) put rows q + 4 on rows
//   q and rows q + 8 on rows q + 12: 2-way on every read).  Stores: the eight lanes of a ds_write_b128 group write one row's 64 B of
//   plane 0 and of plane 1; the planes are a multiple of 128 B apart, so without the r ^ 1 both landed on the same 16 banks.
//   Wave tiling: with 16-cycle MFMAs the loop is bound by LDS bandwidth, not by the matrix pipe (measured: the
//   same time with the MFMAs removed), so the waves are tiled 2 x 2 instead of 1 x 4: wave = (row half rh, column pair cp)
//   owns row tiles 4 rh .. 4 rh + 4 (tile 4 is computed by both halves -- 10 % more MFMAs, no divergence) x column tiles
//   2 cp, 2 cp + 1: 14 fragment reads per wave and chunk instead of 20.  Only the park below knows the tiling; the epilogue
//   reads the parked block.
//   Fragment sets: F0 = {A_hi[5], B_hi[2], B_lo[2]}, F1 = {A_lo[5]}.  Chunk: park k+1 | read F1(k) | MFMA A_hi.B_hi, A_hi.B_lo |
//   barrier | read F0(k+1) | MFMA A_lo.B_hi(k)  -- B_hi lives in two register sets that alternate per chunk.
    const int nk = g.D / SC_BK;
    const unsigned rowbytes = (unsigned)g.D * 4u;      // per 32-wide chunk: 64 B hi | 64 B lo
    const int64_t n_img_rows = g.Ni * SC_R;
    const char *abase = reinterpret_cast<const char *>(g.img_bf) + img0 * SC_R * (int64_t)rowbytes;
    const char *bbase = reinterpret_cast<const char *>(g.wt_bf) + ct * SC_NT * (int64_t)rowbytes;
    constexpr unsigned BPLANE = SC_ROWS * 64u;          // 14 336 B: one plane of one buffer
    constexpr unsigned STAGE_BYTES = 2 * BPLANE;        // 28 672 B, the size of the fp32 stage buffer
    static_assert(STAGE_BYTES == SC_PLANES * SC_ROWS * 16u, "bf16 staging must fit the fp32 stage buffers");
    unsigned va0, va1, va2, va3, va4, vb0, vb1;         // per-lane global byte offsets
    unsigned la0, la1, la2, la3, la4, lb0, lb1;         // per-lane LDS byte addresses (buffer 0)
    {
        const int p = tid & 7, r8 = tid >> 3;           // p = (plane, granule): 8 x 16 B = the 128 B of one row's chunk
        const unsigned pl = (unsigned)p >> 2, gq = (unsigned)p & 3u;
        auto a_off = [&](int row) -> unsigned {
            const bool ok = img0 * SC_R + row < n_img_rows;
            return (ok ? (unsigned)row : 0u) * rowbytes + (unsigned)p * 16u;
        };
        auto l_off = [&](int lrow) -> unsigned {
            return pl * BPLANE + ((unsigned)lrow ^ pl) * 64u + ((gq ^ ((0u - ((unsigned)lrow >> 2)) & 3u)) * 16u);
        };
        va0 = a_off(r8); va1 = a_off(r8 + 32); va2 = a_off(r8 + 64); va3 = a_off(r8 + 96);
        la0 = l_off(r8); la1 = l_off(r8 + 32); la2 = l_off(r8 + 64); la3 = l_off(r8 + 96);
        const int r4 = (tid & 127) >> 3;
        if (wave < 2) { va4 = a_off(128 + r4); la4 = l_off(128 + r4); }
        else          { va4 = (unsigned)p * 16u; la4 = l_off(SC_MT + SC_NT + r4); }   // dump rows 208..223
        vb0 = (unsigned)r8 * rowbytes + (unsigned)p * 16u;        lb0 = l_off(SC_MT + r8);
        vb1 = (unsigned)(r8 + 32) * rowbytes + (unsigned)p * 16u; lb1 = l_off(SC_MT + r8 + 32);
    }
    // fragment reads: lane (row fi, k group fg) takes granule fg of its row; (row >> 2) & 3 == (fi >> 2) & 3 for every tile
    constexpr int WR = 5, WC = 2;                       // MFMA tiles per wave: 5 row tiles x 2 column tiles
    const int rh = wave & 1, cp = wave >> 1;
    const unsigned fgs = (((unsigned)fg ^ ((0u - ((unsigned)fi >> 2)) & 3u)) * 16u);
    const unsigned fsw = (unsigned)fi * 64u + fgs, fsw_lo = ((unsigned)fi ^ 1u) * 64u + fgs;      // plane 1: rows stored at r ^ 1
    const unsigned ra_h = fsw + (unsigned)(4 * rh * 16) * 64u;
    const unsigned ra_l = fsw_lo + (unsigned)(4 * rh * 16) * 64u + BPLANE;
    const unsigned rb_h = fsw + (unsigned)(SC_MT + 2 * cp * 16) * 64u;
    const unsigned rb_l = fsw_lo + (unsigned)(SC_MT + 2 * cp * 16) * 64u + BPLANE;
    char *const lds = smem_raw;

    constexpr bool F16 = (PREC & 2) != 0;
    constexpr bool DUAL = F16;
    f32x4 acc[WR][WC], acx[WR][WC];                     // acx: the scaled cross terms of the fp16 variant (unused for bf16)
#pragma unroll
    for (int i = 0; i < WR; ++i)
#pragma unroll
        for (int j = 0; j < WC; ++j) {
            acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            acx[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }

    f32x4 sa0, sa1, sa2, sa3, sa4, sa5, sa6;   // register stage A
    f32x4 sb0, sb1, sb2, sb3, sb4, sb5, sb6;   // register stage B
#define SC_LDG(dst, base, voff)                                                                    \
    asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(dst) : "v"(voff), "s"(base) : "memory");
#define SC_GLOAD(P, KC)                                                                            \
    {                                                                                              \
        const char *ab_ = abase + (int64_t)(KC) * (SC_BK * 4);                                     \
        const char *bb_ = bbase + (int64_t)(KC) * (SC_BK * 4);                                     \
        SC_LDG(P##0, ab_, va0) SC_LDG(P##1, ab_, va1) SC_LDG(P##2, ab_, va2) SC_LDG(P##3, ab_, va3) \
        SC_LDG(P##4, ab_, va4) SC_LDG(P##5, bb_, vb0) SC_LDG(P##6, bb_, vb1)                       \
    }
#define SC_VMWAIT(P, N)                                                                            \
    asm volatile("s_waitcnt vmcnt(" #N ") ; covers %0 %1 %2 %3 %4 %5 %6"                           \
                 : "+v"(P##0), "+v"(P##1), "+v"(P##2), "+v"(P##3), "+v"(P##4), "+v"(P##5), "+v"(P##6)::"memory");
#define SC_STS(addr, BUF, v) (*reinterpret_cast<f32x4 *>(lds + (addr) + (BUF) * STAGE_BYTES) = (v))
#define SC_LSTORE(P, BUF)                                                                          \
    {                                                                                              \
        SC_STS(la0, BUF, P##0); SC_STS(la1, BUF, P##1); SC_STS(la2, BUF, P##2); SC_STS(la3, BUF, P##3); \
        SC_STS(la4, BUF, P##4); SC_STS(lb0, BUF, P##5); SC_STS(lb1, BUF, P##6);                    \
    }
#define SC_LDS4(addr) (*reinterpret_cast<const f32x4 *>(lds + (addr)))
#define SC_MFMA(A, B, C)                                                                           \
    if constexpr (F16) C = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, (A)), __builtin_bit_cast(f16x8_t, (B)), C, 0, 0, 0); \
    else C = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, (A)), __builtin_bit_cast(bf16x8_t, (B)), C, 0, 0, 0);
    f32x4 fah[WR], fal[WR], bh0[WC], bh1[WC], fbl[WC];
#define SC_MM(A, B, ACC)                                                                           \
    _Pragma("unroll") for (int i = 0; i < WR; ++i)                                                 \
        _Pragma("unroll") for (int j = 0; j < WC; ++j) { SC_MFMA(A[i], B[j], ACC[i][j]) }
#define SC_SGB(mask, n) __builtin_amdgcn_sched_group_barrier(mask, n, 0);
#define SC_CHUNK(P, CUR, NXT, KC, BHC, BHN)                                                        \
    {                                                                                              \
        SC_VMWAIT(P, 7)                                                                            \
        SC_LSTORE(P, NXT)                                                                          \
        SC_GLOAD(P, ((KC) + 3 < klast ? (KC) + 3 : klast))                                         \
        _Pragma("unroll") for (int i = 0; i < WR; ++i)                                             \
            fal[i] = SC_LDS4(ra_l + (CUR) * STAGE_BYTES + i * 1024);                               \
        SC_MM(fah, BHC, acc) if constexpr (DUAL) { SC_MM(fah, fbl, acx) } else { SC_MM(fah, fbl, acc) }                           \
        _Pragma("unroll") for (int i_ = 0; i_ < 7; ++i_) { SC_SGB(0x008, 1) SC_SGB(0x200, 1) }     \
        _Pragma("unroll") for (int i_ = 0; i_ < 5; ++i_) { SC_SGB(0x008, 1) SC_SGB(0x100, 1) }     \
        SC_SGB(0x008, 8)                                                                           \
        __syncthreads();                                                                           \
        _Pragma("unroll") for (int i = 0; i < WR; ++i)                                             \
            fah[i] = SC_LDS4(ra_h + (NXT) * STAGE_BYTES + i * 1024);                               \
        _Pragma("unroll") for (int j = 0; j < WC; ++j) {                                           \
            BHN[j] = SC_LDS4(rb_h + (NXT) * STAGE_BYTES + j * 1024);                               \
            fbl[j] = SC_LDS4(rb_l + (NXT) * STAGE_BYTES + j * 1024);                               \
        }                                                                                          \
        if constexpr (DUAL) { SC_MM(fal, BHC, acx) } else { SC_MM(fal, BHC, acc) }                                                 \
        _Pragma("unroll") for (int i_ = 0; i_ < 9; ++i_) { SC_SGB(0x008, 1) SC_SGB(0x100, 1) }     \
        SC_SGB(0x008, 1)                                                                           \
        if ((KC) >= klast) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   /* last chunk: see the drain note below */ \
    }

    const int klast = nk - 1;
    SC_GLOAD(sa, 0)
    SC_GLOAD(sb, (1 < klast ? 1 : klast))
    SC_VMWAIT(sa, 7)
    SC_LSTORE(sa, 0)
    SC_GLOAD(sa, (2 < klast ? 2 : klast))
    __syncthreads();
    SC_TICK(4)   // prologue: first operand chunk in LDS
#pragma unroll
    for (int i = 0; i < WR; ++i) fah[i] = SC_LDS4(ra_h + i * 1024);
#pragma unroll
    for (int j = 0; j < WC; ++j) {
        bh0[j] = SC_LDS4(rb_h + j * 1024);
        fbl[j] = SC_LDS4(rb_l + j * 1024);
        bh1[j] = bh0[j];
    }
    for (int kc = 0; kc < nk; kc += 2) {
        SC_CHUNK(sb, 0, 1, kc, bh0, bh1)
        if (kc + 1 >= nk) break;
        SC_CHUNK(sa, 1, 0, kc + 1, bh1, bh0)
    }
    // The tail prefetches (re-loads of the last chunk, never consumed) are drained INSIDE the last chunk, before the loop is left:
    // their destination registers hold dead values once the loop exits, the compiler hands them to the copies it places on the
    // exit edges, and load data arriving late then overwrites those (seen with the fp16x3 build: sporadic garbage, only with two
    // workgroups per CU).  Naming the stage registers as operands of a wait after the loop instead costs 56 live VGPRs at the
    // exit and makes the fp32 kernel spill -- and spill code in the loop breaks the manual vmcnt counting.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#undef SC_LDG
#undef SC_GLOAD
#undef SC_STS
#undef SC_VMWAIT
#undef SC_LSTORE
#undef SC_LDS4
#undef SC_MFMA
#undef SC_MM
#undef SC_CHUNK
#undef SC_SGB

    __syncthreads();
    SC_TICK(0)   // prologue + main loop
    // C/D layout of a 16 x 16 tile: lane (fi = column, fg) holds rows 4 fg .. 4 fg + 3.  Row tile 4 is parked by both row
    // halves with identical values.
#pragma unroll
    for (int j = 0; j < WC; ++j) {
        float *colp = &sm.arawt[(2 * cp + j) * 16 + fi][4 * rh * 16 + fg * 4];
#pragma unroll
        for (int i = 0; i < WR; ++i)
            *reinterpret_cast<f32x4 *>(colp + i * 16) =
                F16 ? (acc[i][j] + acx[i][j] * (1.f / 2048.f)) * (1.f / 16777216.f) : acc[i][j];      // 2^-24: both operands carry 2^12
    }
    __syncthreads();
    SC_TICK(1)   // park
