// uva_sub10_body.hip.h -- the body that sub10_kernel and sub10_kernel16 share (csrc/uva_sub10.hip.h includes it inside each of the
// two, after `typedef ... A;` for the kernel's argument block `a` and the declaration of `smem`).  Text and not a function: passed
// through a function template the u8 kernel compiled to other instructions than before (four commuted adds, one address formed
// differently), and the kernel is to stay what was measured.
    const Sub10Lds L = sub10_lds<sizeof(typename Sub10Sample<A>::type) == 2>(smem);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int nrows = __builtin_amdgcn_readfirstlane(a.nrows[blockIdx.x]);
    if (nrows <= 0) return;
    // this workgroup's row descriptors live in LDS, 8 bytes each: {32 ((frame << 16) + y + 16) + 2 dist + emit, x0} (dist: rows between y and the nearest row
    // of its segment that is written out, 0..10 -- layer s is needed where dist <= 9 - s); every wave reads one (or two) per step
    {
        const uint4* const grows = a.rows + (size_t)blockIdx.x * a.max_rows;
        for (int i = threadIdx.x; i < nrows; i += 64 * S10_NW) {
            const uint4 e = grows[i];
            L.rows[i] = make_int2(((int)((e.z >> 8) << S10_FSHIFT) + (int)e.x + S10_YBIAS) * 32 + (int)(e.w & 15u) * 2 + (int)(e.z & 1), (int)e.y);
        }
    }
    // rings start as zeros (margins and pipeline fill are never written: no NaN patterns may sit there)
    for (int i = threadIdx.x; i < ((S10_NL - 1) * S10_RINGB + S10_URINGB) / 16; i += 64 * S10_NW)
        ((uint4*)smem)[i] = make_uint4(0, 0, 0, 0);
    if (wave < S10_NL && lane < 32) {
        L.prm[wave * 96 + lane] = a.bias[wave][lane];
        L.prm[wave * 96 + 32 + lane] = wave + 1 < S10_NL ? a.slope[wave][lane] : 0.f;
    }
    __syncthreads();
    // every wave runs the same number of steps = barriers, whatever code it sits in
    const int nsteps = (nrows + S10_DRAIN + 1) & ~1;
    // Waves w, w+4, w+8 share a SIMD: two trunk layers and one half of the first or the last layer each -- the same
    // MFMA and VALU load on all four.  (No s_setprio: with the light waves halved, raising them or the trunk waves
    // measured 2 % slower than leaving the arbiter alone, profiles/r02_sub10_experiments.txt.)
#define S10_BAL 1
    // Round 5 (profiles/r05_ab_results.txt block 19): only columns 10..69 of the last layer are stored, so trunk layer 8 is needed
    // on columns 9..70 and layer 7 on 8..71 -- 64 columns, FOUR fragments at a column shift of 8 (an even number of 16-byte units:
    // the conflict-free read recipe holds), where every layer computed all five.  The last layer likewise: four fragments, two per
    // wave instead of three and two.  What a SIMD carries was 3 818 / 3 458 / 3 744 / 3 224 ticks per row (head 3 fragments, head 2,
    // tail 3, tail 2 beside two five-fragment trunk waves each); now the tail halves sit beside the five-fragment layers (waves
    // 8, 9) and the head halves beside the two four-fragment ones (waves 10, 11).  The rings' columns 0..7 and 72..79 of layers 7
    // and 8 stay at the zeros the kernel starts with; what reads them is never stored.
#define S10_MAP 0       // A/B builds (block 22): 1 = the first layer's three-fragment half on wave 11 instead of 10; 2 = the four-fragment
                              // layers on the OLDER waves of their SIMDs (waves 2, 3 = layers 7, 8; waves 6, 7 = layers 3, 4)
    if (wave < 6) sub10_body<false, 0, 5>(a, L, wave, wave + 1, lane, nrows, nsteps);
    else if (wave < 8) sub10_body<false, 0, 4, 8>(a, L, wave, wave + 1, lane, nrows, nsteps);
    else if (wave == 8) sub10_body<true, 0, 2, 8>(a, L, wave, S10_NL - 1, lane, nrows, nsteps);
    else if (wave == 9) sub10_body<true, 2, 4, 8>(a, L, wave, S10_NL - 1, lane, nrows, nsteps);
    else if (wave == (S10_MAP == 1 ? 11 : 10)) sub10_head<0>(a, L, wave, lane, nrows, nsteps);
    else sub10_head<1>(a, L, wave, lane, nrows, nsteps);
