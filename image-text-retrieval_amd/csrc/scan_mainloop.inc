// Textually included INSIDE scan_xattn_body<0> (scan_xattn.hip; SGRAF runs the same kernel in emit mode).
// Computes the raw dot products A[144 region rows x 64 word columns] of one (4-image, column-tile) workgroup
// with fp32 MFMAs and parks them transposed in LDS (sm.arawt[column][row]).
// Expects in scope: g.{img, wtiled, D, Ni, dbg_cycles}, img0, ct, tid, lane, wave, fi, fg, smem_raw, sm (ScanSmem-like:
// .stage at offset 0 of the dynamic LDS block, .arawt aliasing it), tick_ (debug timer).
// Leaves the block parked in sm.arawt (everything it declares is local to the including block).
    // ---- main loop: raw dot products A[144 x 64] over K = D ------------------------------
    // On gfx950 the fp32 MFMA shares the vector ALU with ordinary VALU work (tools/ubench: an MFMA wave and
    // a VALU wave on one SIMD take the SUM of their times), so every VALU instruction in this loop is paid
    // in matrix throughput.  All addressing is therefore loop-invariant:
    //   * global loads use  uniform 64-bit base (SGPR, advanced by a scalar add per chunk) + per-lane 32-bit
    //     byte offset (VGPR, fixed);  7 passes per chunk, each homogeneous in its base:
    //       A0..A3: image rows 0..127 | A4: rows 128..143 (waves 0,1; waves 2,3 re-load row 0 into the 16
    //       dump rows) | B0,B1: the 64 word columns of this tile;
    //   * LDS stores / fragment reads use a per-lane byte address (VGPR, fixed) + immediate offset (buffer,
    //     row tile): (m*16 + fi) ^ p == m*16 + (fi ^ p) because p < 8.
    // Rows that do not exist (image tail) re-read row 0: their outputs are never consumed.
    const int nk = g.D / SC_BK;  // D % 32 == 0 is checked on the host
    const unsigned rowbytes = (unsigned)g.D * 4u;
    const int64_t n_img_rows = g.Ni * SC_R;
    const char *abase = reinterpret_cast<const char *>(g.img) + img0 * SC_R * (int64_t)rowbytes;
    const char *bbase = reinterpret_cast<const char *>(g.wtiled) + ct * SC_NT * (int64_t)rowbytes;
    const int64_t bpass = 32 * (int64_t)rowbytes;    // B pass 1 = B pass 0 + 32 rows: a second scalar base, no second VGPR
    unsigned va0, va1, va2, va3, va4, vb0;            // per-lane global byte offsets
    unsigned la0, la4;                                // per-lane LDS byte addresses (buffer 0).  Every other pass is la0 + an
                                                      // immediate: (c + r8) ^ p == c + (r8 ^ p) for c % 8 == 0 (p < 8), so
                                                      // l_off(c + r8) = la0 + 16 c
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char *)smem_raw;   // LDS byte address of the block
    {
        const int p = tid & 7, r8 = tid >> 3;          // 32 rows per pass
        auto a_off = [&](int row) -> unsigned {
            const bool ok = img0 * SC_R + row < n_img_rows;
            return (ok ? (unsigned)row : 0u) * rowbytes + p * 16u;
        };
        auto l_off = [&](int row) -> unsigned { return lds0 + (unsigned)(p * SC_ROWS + (row ^ p)) * 16u; };
        va0 = a_off(r8); va1 = a_off(r8 + 32); va2 = a_off(r8 + 64); va3 = a_off(r8 + 96);
        la0 = l_off(r8);
        const int r4 = (tid & 127) >> 3;                // 16 rows in the fifth A pass
        if (wave < 2) { va4 = a_off(128 + r4); la4 = l_off(128 + r4); }
        else          { va4 = p * 16u;          la4 = l_off(SC_MT + SC_NT + r4); }   // dump rows 208..223
        vb0 = (unsigned)r8 * rowbytes + p * 16u;
    }
    // fragment read addresses: plane p = 4q + fg, physical row (fi ^ p) (+ m*16, + 144 + wave*16 for B)
    const unsigned ra0 = lds0 + (unsigned)((fg) * SC_ROWS + (fi ^ fg)) * 16u;
    const unsigned ra1 = lds0 + (unsigned)((4 + fg) * SC_ROWS + (fi ^ (4 + fg))) * 16u;
    const unsigned rb0 = ra0 + (unsigned)(SC_MT + wave * 16) * 16u;
    const unsigned rb1 = ra1 + (unsigned)(SC_MT + wave * 16) * 16u;
    // Two register stages: chunk kc+2 is in flight while chunk kc is multiplied and chunk kc+1 is parked in the other LDS
    // buffer, so an HBM miss has ~2 chunks (>= 4.6k cycles) to land.  hipcc's own s_waitcnt bookkeeping merged the two
    // stages into vmcnt(0) at the loop header (a full L2 / HBM latency exposed every chunk), so the loads are counted by
    // hand: when stage P is parked, the 7 loads of the OTHER stage (issued one chunk later) may still be in flight ->
    // s_waitcnt vmcnt(7).  A load hidden from hipcc has, to hipcc, a destination that is written when the asm statement
    // ends -- free to be copied, spilled or reused while the data is in flight (cdna_hip_programming.md 5.7); at this kernel's
    // register budget every C++-level restructuring made the allocator do exactly that inside the loop (round 2,
    // tools/audit_asm_loads.py).  So the whole loop -- prologue, K loop, peeled tail, park -- is ONE asm statement with
    // hand-allocated registers (generated: tools/gen_scan_mainloop.py; v[64:235], s[80:86] are listed as clobbered, hipcc
    // keeps its values elsewhere), nothing is in flight when it ends, and the MFMA / memory interleave is the one written
    // there: one memory instruction behind each of the first MFMAs of a half chunk, the 7 park stores behind every OTHER
    // one, with the fragment reads between them.  tools/ubench/mfma_pipe: 3091 cycles per chunk issued in a clump, 2456 with
    // the 7 stores behind 7 consecutive MFMAs (the four waves' 16-byte LDS stores, ~13 LDS cycles each, then outrun the LDS
    // and stall MFMA issue when a wave has no partner on its SIMD), 2358 as it is now, against 2304 of pure MFMA issue.
    const unsigned park_addr = lds0 + (unsigned)(((wave * 16 + fi) * SC_LDT + fg * 4) * 4);   // &sm.arawt[wave*16 + fi][fg*4]
    if (nk >= 3) {
        const char *bbase2 = bbase + bpass;
        const int nmain = nk - 3;
#include "scan_mainloop_asm.inc"
        SC_TICK(4)   // (the prologue is inside the statement: not timed separately any more)
        SC_TICK(0)   // prologue + main loop + park
    } else {
        // D = 32 or 64 (toy sizes): one or two chunks, compiler-managed loads, no pipeline -- load, park, multiply
        f32x4 acc[SC_MTILES];
#pragma unroll
        for (int m = 0; m < SC_MTILES; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
        char *const lds = smem_raw;
        for (int kc = 0; kc < nk; ++kc) {
            const char *ab_ = abase + (int64_t)kc * (SC_BK * 4), *bb_ = bbase + (int64_t)kc * (SC_BK * 4);
            const f32x4 t0 = *reinterpret_cast<const f32x4 *>(ab_ + va0), t1 = *reinterpret_cast<const f32x4 *>(ab_ + va1);
            const f32x4 t2 = *reinterpret_cast<const f32x4 *>(ab_ + va2), t3 = *reinterpret_cast<const f32x4 *>(ab_ + va3);
            const f32x4 t4 = *reinterpret_cast<const f32x4 *>(ab_ + va4), t5 = *reinterpret_cast<const f32x4 *>(bb_ + vb0);
            const f32x4 t6 = *reinterpret_cast<const f32x4 *>(bb_ + bpass + vb0);
            __syncthreads();                                 // every wave is done reading the previous chunk
            *reinterpret_cast<f32x4 *>(lds + (la0 - lds0)) = t0;
            *reinterpret_cast<f32x4 *>(lds + (la0 - lds0) + 32 * 16) = t1;
            *reinterpret_cast<f32x4 *>(lds + (la0 - lds0) + 64 * 16) = t2;
            *reinterpret_cast<f32x4 *>(lds + (la0 - lds0) + 96 * 16) = t3;
            *reinterpret_cast<f32x4 *>(lds + (la4 - lds0)) = t4;
            *reinterpret_cast<f32x4 *>(lds + (la0 - lds0) + SC_MT * 16) = t5;
            *reinterpret_cast<f32x4 *>(lds + (la0 - lds0) + (SC_MT + 32) * 16) = t6;
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const unsigned ra = (q ? ra1 : ra0) - lds0, rb = (q ? rb1 : rb0) - lds0;
                const float4 fb = *reinterpret_cast<const float4 *>(lds + rb);
#pragma unroll
                for (int m = 0; m < SC_MTILES; ++m) {
                    const float4 fa = *reinterpret_cast<const float4 *>(lds + ra + m * 256);
                    acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa.x, fb.x, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa.y, fb.y, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa.z, fb.z, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa.w, fb.w, acc[m], 0, 0, 0);
                }
            }
        }
        __syncthreads();
        SC_TICK(4)
        SC_TICK(0)
        {
            float *colp = &sm.arawt[wave * 16 + fi][fg * 4];
#pragma unroll
            for (int m = 0; m < SC_MTILES; ++m) *reinterpret_cast<f32x4 *>(colp + m * 16) = acc[m];
        }
        __syncthreads();
    }
    SC_TICK(1)   // park

    // ---- epilogue ------------------------------------------------------------------------------------------
    // Next to a wave that streams 32-cycle fp32 MFMAs (the other workgroup of this CU) every VALU instruction
    // of this wave waits for an MFMA slot, so the epilogue is built to issue few instructions: the block is
    // parked TRANSPOSED ([word column][region row]) so that every access below is a 16-byte LDS access, and
    // the two reductions with real arithmetic (first-norm statistics, ||ctx||^2) run on the matrix core.
