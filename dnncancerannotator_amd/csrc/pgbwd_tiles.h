// pgbwd_tiles.h -- the tile loop of k_pgbwd (kernels_mfma.hip), included INSIDE that kernel's body, once per copy of the loop:
//   PGBWD_ROLE 0   every wave runs this copy (all instantiations without CW)
//   PGBWD_ROLE 1   CW: the copy of the data-gradient waves (+ the riding transposed conv)
//   PGBWD_ROLE 2   CW: the copy of the weight-gradient waves
// The copies of CW execute the same barriers.  Text, not a function: the kernel's locals are used by name, and the instantiations
// without CW compile to what they were when this loop stood in the kernel.
#pragma unroll 1
    while (tile < ntiles) {
        constexpr int ROLE = PGBWD_ROLE;
        int b, x0, y0;
        decode(tile, b, x0, y0);
        STAMP(0);
        if constexpr (PF) {
            pf_commit_pooled();
            lds_barrier();
            pf_transform(okg);
        }
        if constexpr (CW) {
            float4* dump = lds4 + TSUM0 + TSUM4 + tid;
            tile_commit_all<CO, TW, NT>(preg, okg, lds4, dump, tid);
#pragma unroll
            for (int s = 0; s < NSRC; ++s) tile_commit_all<C, TW, NT>(prex[s], okx, lds4 + TGg::N4 + s * TGx::N4, dump, tid);
        } else {
            tile_commit<CO, TW, NT>(preg, okg, lds4, tid);
#pragma unroll
            for (int s = 0; s < NSRC; ++s) tile_commit<C, TW, NT>(prex[s], okx, lds4 + TGg::N4 + s * TGx::N4, tid);
        }
        lds_barrier();      // (barrier 1 of 2 per tile: every copy of this loop executes it, whatever its ROLE)
        constexpr int GOFF = 0, XOFF = TGg::N4 * 4;      // float indices of the dz / x tiles
        const float* gl = ldsf + GOFF;
        const float* xl = ldsf + XOFF;
        STAMP(1);
        // TCF: a data-gradient wave owns the column block tx = wave of the tile (32 pixels, all TH rows) = 16 x TH/2 pixels of the
        // transposed conv's input, one per lane; their 6 channels are fetched now (ahead of the prefetch: vmcnt retires in order)
        float tin[TCF ? 6 : 1];
        if constexpr (TCF) {
            if (ROLE == 1 || (ROLE == 0 && wave < NWD)) {
                const int pr = lane >> 4, pc = lane & 15;
                const float* ip = p.tc_in + ((((size_t)b * (p.H >> 1) + (y0 >> 1) + pr) * (p.W >> 1)) + (x0 >> 1) + wave * 16 + pc) * 6;
#pragma unroll
                for (int ci = 0; ci < 6; ++ci) tin[ci] = ip[ci];
            }
        }
        // TCM: this thread's float4 of the transposed conv's input tile (ahead of the prefetch, as tin)
        float4 txl = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (TCM) {
            if (tid < XLT4) {
                const int r = tid / (LWt * 3), c = tid - r * (LWt * 3);
                txl = reinterpret_cast<const float4*>(p.tc_in)[(((size_t)b * (p.H >> 1) + (y0 >> 1) + r) * (p.W >> 1) + (x0 >> 1)) * 3 + c];
            }
        }
        const int next = tile + gridDim.x;
        if (CW || next < ntiles) {      // CW: on every tile -- past the end the same tile again, which nobody commits
            int nb, nx0, ny0;
            decode(CW && next >= ntiles ? tile : next, nb, nx0, ny0);
            okg = tile_issue<CO, TW, NT>(preg, mpg, p.dz, nb, nx0, ny0, p.B, p.H, p.W);
            pf_issue(nb, nx0, ny0);
#pragma unroll
            for (int s = 0; s < NSRC; ++s) okx = tile_issue<C, TW, NT>(prex[s], mpx, p.x[s], nb, nx0, ny0, p.B, p.H, p.W);
        }

        STAMP(2);
        // ---- data gradient: conv of dz with the flipped kernel; M-tiles of 16 groups x Gd pixels
        if (DGRAD && ROLE != 2 && !(DBG_FLAGS(p) & 1)) {
            // M-tiles of this wave: t = wave + 4j, j < MTX*TH/4; NCH of them are processed with interleaved MFMA chains
            constexpr int PERW = Wc::MTX * TH / NWD;
            constexpr int NCH = (VW && NSRC == 1) ? 2 : (PERW >= 4 ? 4 : PERW);      // (VW, one source: two chains keep the kernel under 128 registers)
#pragma unroll 1
            for (int j0 = 0; j0 < (ROLE == 0 && VW && wave >= NWD ? 0 : PERW); j0 += NCH) {
#pragma unroll
                for (int ps = 0; ps < NPASS; ++ps) {
                    f32x4 d[NCH];
                    int txs[NCH], tys[NCH];
#pragma unroll
                    for (int i = 0; i < NCH; ++i) {
                        const int t = wave + NWD * (j0 + i);
                        txs[i] = t % Wc::MTX;
                        tys[i] = t / Wc::MTX;
                        d[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                    }
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                        for (int k = 0; k < SRd; ++k)
#pragma unroll
                            for (int i = 0; i < NCH; ++i)
                                d[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                                    gl[(tys[i] + dy) * LSg + TGg::LEAD + (txs[i] * 16 + m16) * (Gd * CO) + q + 4 * k],
                                    breg[ps * KSd + dy * SRd + k], d[i], 0, 0, 0);
                    // transpose D through LDS: per destination the M-tile's gradient row is 16 groups x (Gd*CS)
                    // contiguous floats; then 16-byte masked / accumulated stores
                    constexpr int SPL = (NSRC == 2 && NPASS == 1) ? 2 : 1;     // destinations covered by this pass
                    constexpr int CS = COd / SPL;                              // channels per destination (== C)
                    constexpr int PER4 = 16 * Gd * CS / 4;                      // float4's per destination row segment
#pragma unroll
                    for (int i = 0; i < NCH; ++i) {
                        const int tx = txs[i], ty = tys[i], y = y0 + ty;
                        if (n < Nd) {
                            const int sp = cod / CS, cs = cod - sp * CS;
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                orow[sp * (16 * Gd * CS) + (4 * q + r) * (Gd * CS) + dxp * CS + cs] = d[i][r];
                        }
                        __builtin_amdgcn_wave_barrier();
                        const int sp = lane / PER4, i4 = lane - sp * PER4;
                        const int src = NPASS == 2 ? ps : sp;
                        // (the destination is picked with selects between kernel arguments: indexing p.dx / p.acc / p.mask with a
                        //  per-lane value made the compiler FETCH them from the kernarg segment with vector loads, and the
                        //  s_waitcnt vmcnt(0) behind each of those also drained the next tile's prefetch -- a full HBM round
                        //  trip per M-tile, 2 400 cycles around 480 cycles of MFMAs)
                        float* dxs;
                        int accs, masks;
                        if constexpr (NPASS == 2) { dxs = ps ? p.dx[1] : p.dx[0]; accs = ps ? p.acc[1] : p.acc[0]; masks = ps ? p.mask[1] : p.mask[0]; }
                        else if constexpr (SPL == 2) { dxs = sp ? p.dx[1] : p.dx[0]; accs = sp ? p.acc[1] : p.acc[0]; masks = sp ? p.mask[1] : p.mask[0]; }
                        else { dxs = p.dx[0]; accs = p.acc[0]; masks = p.mask[0]; }
                        const int f0 = (x0 + tx * 16 * Gd) * C + 4 * i4;        // float index within the image row
                        if constexpr (CW) {
                            // lanes [0, PER4): the first source's row into the LDS tile; lanes [PER4, 2 PER4): the second source's row
                            // to memory, masked with act'(x) from the staged tile; the rest: a store to nowhere.  (The launcher sends
                            // an accumulating destination to the kernel without CW.)
                            // Lanes [2 PER4, 64) have no row: they read the first float4 of this wave's row (and below, the mask
                            // words of their i4) so that no lane reads LDS words another wave writes; what they hold is never stored.
                            float4 v = reinterpret_cast<const float4*>(orow)[lane < 2 * PER4 ? lane : 0];
                            if (lane < PER4) dta4[(ty * 4 + tx) * 24 + i4] = v;
                            if (p.mask[1]) {
                                const float4 xv = *reinterpret_cast<const float4*>(
                                    xl + (TGx::N4 * 4) + (ty + 1) * LSx + TGx::HL + tx * 16 * Gd * C + 4 * i4);
                                v.x *= xv.x > 0.f ? 1.0f : p.alpha;
                                v.y *= xv.y > 0.f ? 1.0f : p.alpha;
                                v.z *= xv.z > 0.f ? 1.0f : p.alpha;
                                v.w *= xv.w > 0.f ? 1.0f : p.alpha;
                            }
                            // the second source's gradient of this tile's image as a raw buffer (byte offsets within the image)
                            const __amdgpu_buffer_rsrc_t rs_dx1 = __builtin_amdgcn_make_buffer_rsrc(
                                (void*)(p.dx[1] + (size_t)b * p.H * p.W * C), 0, p.H * p.W * C * 4, PG_RSRC);
                            const unsigned off = sp == 1 ? ((unsigned)y * (unsigned)(p.W * C) + (unsigned)f0) * 4u : PG_NOWHERE;
                            store16<DNNCA_STORE_AUX_MFMA_BWD>(rs_dx1, off, v);
                        } else if (TCF && sp == 0) {
                            // the first source's gradient (= the transposed conv's output gradient) stays in LDS (whole tiles only)
                            if (lane < PER4) dta4[(ty * 4 + tx) * 24 + i4] = reinterpret_cast<const float4*>(orow)[lane];
                        } else if (TCM && src == 0) {
                            if (lane < PER4) lds4[TCM0 + (ty * Wc::MTX + tx) * PER4 + i4] = reinterpret_cast<const float4*>(orow)[lane];
                        } else if (lane < SPL * PER4 && f0 < p.W * C && y < p.H) {
                            float4 v = reinterpret_cast<const float4*>(orow)[lane];
                            float* dst = dxs + ((size_t)b * p.H + y) * p.W * C + f0;
                            if (accs) {
                                const float4 o = *reinterpret_cast<const float4*>(dst);
                                v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
                            }
                            if (masks) {
                                const float4 xv = *reinterpret_cast<const float4*>(
                                    xl + src * (TGx::N4 * 4) + (ty + 1) * LSx + TGx::HL + tx * 16 * Gd * C + 4 * i4);
                                v.x *= xv.x > 0.f ? 1.0f : p.alpha;
                                v.y *= xv.y > 0.f ? 1.0f : p.alpha;
                                v.z *= xv.z > 0.f ? 1.0f : p.alpha;
                                v.w *= xv.w > 0.f ? 1.0f : p.alpha;
                            }
                            if constexpr (SPL == 1) {
                                // one destination per pass (uniform): the store goes through this image's raw buffer
                                const __amdgpu_buffer_rsrc_t rs_dx = store_rsrc(dxs + (size_t)b * p.H * p.W * C, (unsigned)(p.H * p.W * C) * 4u);
                                store16<DNNCA_STORE_AUX_MFMA_BWD>(rs_dx, ((unsigned)y * (unsigned)(p.W * C) + (unsigned)f0) * 4u, v);
                            } else {
                                *reinterpret_cast<float4*>(dst) = v;      // (the destination differs between lanes: no uniform descriptor)
                            }
                        }
                        __builtin_amdgcn_wave_barrier();
                    }
                }
            }
        }
        if constexpr (TCM) {
            static_assert(Wc::MTX * (16 * Gd * C / 4) == ROWF / 4, "TCM: the M-tiles of a row tile the gradient row");
            if (tid < XLT4) lds4[TCM0 + DT4 + tid] = txl;
            lds_barrier();                                    // the tile's first-source gradient and the input tile are complete
            // LDS addressing of T1 / T2, recomputed per tile from an opaque copy of the lane id: as loop invariants these seven
            // values would be live across the whole tile loop of a kernel that sits at its register limit
            int lo = lane;
            asm volatile("" : "+v"(lo));
            const int m16 = lo & 15, q = lo >> 4;
            int offT[MBt];
#pragma unroll
            for (int t = 0; t < MBt; ++t) {
                const int k = 16 * t + m16, a = k / KA, kr = k - a * KA;
                offT[t] = k < KTt ? DTF + a * ROWF + 2 * q * C + kr : CST0;
            }
            const int boffT = m16 < CIt ? XLTF + q * CIt + m16 : (m16 == CIt ? CST1 : CST0), bstepT = m16 < CIt ? 4 * CIt : 0;
            const int woffT = m16 < CIt ? TCWF + q * CIt + m16 : CST0, wstepT = bstepT;
            // ---- T1: the transposed conv's data gradient, one M-tile = 16 input pixels of a row
#pragma unroll 1
            for (int mt = wave; mt < NLP / 16; mt += NW) {
                const int li = mt / (LWt / 16), mx = mt - li * (LWt / 16);
                f32x4 d = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int kk = 0; kk < KS1; ++kk)
                        d = __builtin_amdgcn_mfma_f32_16x16x4f32(ldsf[DTF + (2 * li + a) * ROWF + 2 * (mx * 16 + m16) * C + 4 * kk + q],
                                                                 ldsf[woffT + (a * KS1 + kk) * wstepT], d, 0, 0, 0);
                if (m16 < CIt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) orow[(4 * q + r) * CIt + m16] = d[r];
                }
                __builtin_amdgcn_wave_barrier();
                if (lane < 16 * CIt / 4) {
                    float4 v = reinterpret_cast<const float4*>(orow)[lane];
                    if (p.tc_mask) {
                        const float4 xv = lds4[TCM0 + DT4 + (li * LWt + mx * 16) * 3 + lane];
                        v.x *= xv.x > 0.f ? 1.0f : p.tc_alpha;
                        v.y *= xv.y > 0.f ? 1.0f : p.tc_alpha;
                        v.z *= xv.z > 0.f ? 1.0f : p.tc_alpha;
                        v.w *= xv.w > 0.f ? 1.0f : p.tc_alpha;
                    }
                    const __amdgpu_buffer_rsrc_t rs_tc = store_rsrc(p.tc_din + (size_t)b * (p.H >> 1) * (p.W >> 1) * 12, (unsigned)((p.H >> 1) * (p.W >> 1)) * 48u);
                    store16<DNNCA_STORE_AUX_MFMA_BWD>(rs_tc, ((unsigned)((y0 >> 1) + li) * (unsigned)(p.W >> 1) + (unsigned)((x0 >> 1) + mx * 16)) * 48u + lane * 16u, v);
                }
                __builtin_amdgcn_wave_barrier();
            }
            // ---- T2: the transposed conv's weight (+ bias) gradient, K-steps of 4 input pixels dealt to the waves
            if constexpr (TLDS) {
#pragma unroll
                for (int t = 0; t < MBt; ++t) tacc2[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll 1
            for (int st = wave; st < NLP / 4; st += NW) {
                const int sd = ((4 * st) / LWt) * 2 * ROWF + ((4 * st) % LWt) * 2 * C;
                const float bv = ldsf[boffT + st * bstepT];
#pragma unroll
                for (int t = 0; t < MBt; ++t)
                    tacc2[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ldsf[offT[t] + (16 * (t + 1) <= KTt || offT[t] != CST0 ? sd : 0)], bv, tacc2[t], 0, 0, 0);
            }
            if constexpr (TLDS) {
#pragma unroll
                for (int t = 0; t < MBt; ++t) {
                    float4 v = lds4[TSUM0 + (wave * MBt + t) * 64 + lane];
                    v.x += tacc2[t][0]; v.y += tacc2[t][1]; v.z += tacc2[t][2]; v.w += tacc2[t][3];
                    lds4[TSUM0 + (wave * MBt + t) * 64 + lane] = v;
                }
            }
        }
        if constexpr (TCF) {
            // ---- transposed conv backward on the data-gradient waves: lane = one input pixel (pr, pc) of this wave's column block; its
            // 2 x 2 output pixels' gradients are in the LDS tile this wave has just written (DS operations of one wave execute in order)
            if ((ROLE == 1 || (ROLE == 0 && wave < NWD)) && !(DBG_FLAGS(p) & 5)) {          // (tuning builds: DNNCA_DBG bit 2 skips this part alone)
                __builtin_amdgcn_wave_barrier();
                const int pr = lane >> 4, pc = lane & 15;
                const float* dt = reinterpret_cast<const float*>(dta4);
                float din[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    float d6[6];                 // (e, co) of output row 2 pr + a, pixels 2 pc, 2 pc + 1
                    const float* rp = dt + (((2 * pr + a) * 4 + wave) * 24) * 4 + (2 * pc) * 3;
#pragma unroll
                    for (int i = 0; i < 6; ++i) d6[i] = rp[i];
#pragma unroll
                    for (int e = 0; e < 2; ++e)
#pragma unroll
                        for (int co = 0; co < 3; ++co) {
                            const float d = d6[e * 3 + co];
                            tbias[co] += d;
                            const float* wr = tcw + ((a * 2 + e) * 3 + co) * 6;      // uniform address: broadcast reads
#pragma unroll
                            for (int ci = 0; ci < 6; ++ci) {
                                din[ci] = fmaf(d, wr[ci], din[ci]);
                                tacc[((a * 2 + e) * 3 + co) * 6 + ci] = fmaf(d, tin[ci], tacc[((a * 2 + e) * 3 + co) * 6 + ci]);
                            }
                        }
                }
                if (p.tc_mask) {
#pragma unroll
                    for (int ci = 0; ci < 6; ++ci) din[ci] *= tin[ci] > 0.f ? 1.0f : p.tc_alpha;
                }
                // a pixel's 24 bytes as two 12-byte stores through this image's raw buffer.  Plain stores whatever the policy: written
                // through, the 12-byte pieces reach memory one by one (WRITE_SIZE of the launch 37.5 -> 49.7 MB, this tensor twice);
                // as plain stores the L2 merges them into whole lines
                const __amdgpu_buffer_rsrc_t rs_tc = store_rsrc(p.tc_din + (size_t)b * (p.H >> 1) * (p.W >> 1) * 6, (unsigned)((p.H >> 1) * (p.W >> 1)) * 24u);
                const unsigned toff = ((unsigned)((y0 >> 1) + pr) * (unsigned)(p.W >> 1) + (unsigned)((x0 >> 1) + wave * 16 + pc)) * 24u;
                store12<0>(rs_tc, toff, din[0], din[1], din[2]);
                store12<0>(rs_tc, toff + 12u, din[3], din[4], din[5]);
                __builtin_amdgcn_wave_barrier();
            }
        }
        STAMP(3);
        if constexpr (VW) {
            // ---- weight gradient on the vector ALU (waves NWD .. NW-1): lane = one pixel column, sliding window down the rows
            if (ROLE == 2 || (ROLE == 0 && wave >= NWD)) {
                const int wv = wave - NWD;
                if constexpr (NSRC == 1) {
                    // one kernel row dy per wave (27 accumulators): waves 0..2 walk the whole tile, reading input row r + dy for
                    // output row r; wave 3 sums dz (the bias gradient).  Few registers: two blocks per CU stay resident.
#pragma unroll 1
                    for (int h = 0; h < 2; ++h) {
                        const int col = h * 64 + lane;                                       // TW = 128 = two wave widths
                        const float* gb = gl + TGg::HL + col * CO + LSg;                      // dz of (row 0, col)
                        if (wv < 3) {
                            const float* xb = xl + TGx::LEAD + col * C + wv * LSx;           // window row dy = wv of (row 0, col)
                            // two rows in flight: the LDS reads of the next row are issued before the 27 FMAs of this one
                            float xr[2][9], dzv[2][3];
                            auto load = [&](int b, int r) {
#pragma unroll
                                for (int j = 0; j < 9; ++j) xr[b][j] = xb[r * LSx + j];
#pragma unroll
                                for (int co = 0; co < 3; ++co) dzv[b][co] = gb[r * LSg + co];
                            };
                            auto fma27 = [&](int b) {
#pragma unroll
                                for (int j = 0; j < 9; ++j)
#pragma unroll
                                    for (int co = 0; co < 3; ++co) wacc[j * 3 + co] = fmaf(xr[b][j], dzv[b][co], wacc[j * 3 + co]);
                            };
                            load(0, 0);
#pragma unroll 1
                            for (int r = 0; r < TH; r += 2) {
                                load(1, r + 1);
                                fma27(0);
                                load(0, r + 2 < TH ? r + 2 : TH - 1);
                                fma27(1);
                            }
                        } else {
#pragma unroll
                            for (int r = 0; r < TH; ++r)
#pragma unroll
                                for (int co = 0; co < 3; ++co) wacc[co] += gb[r * LSg + co];
                        }
                    }
                } else {
                // two sources: waves 0, 1 take the columns of source 0, waves 2, 3 those of source 1; a lane walks down its
                // column with a sliding 3 x 3 x C window in registers (81 + 3 accumulators)
                const int src = wv >> 1;
                const int col = (wv & 1) * 64 + lane;                                   // TW = 128 = two wave widths
                constexpr int ROWS = TH;
                const int r0 = 0;
                const float* xb = xl + src * (TGx::N4 * 4) + TGx::LEAD + col * C;      // window of pixel (row, col): 9 floats from here
                const float* gb = gl + TGg::HL + col * CO;
                float xw[3][9];
#pragma unroll
                for (int j = 0; j < 9; ++j) { xw[0][j] = xb[r0 * LSx + j]; xw[1][j] = xb[(r0 + 1) * LSx + j]; }
#pragma unroll
                for (int rr = 0; rr < ROWS; ++rr) {
                    const int r = r0 + rr;
                    float dzv[3];
#pragma unroll
                    for (int co = 0; co < 3; ++co) dzv[co] = gb[(r + 1) * LSg + co];
#pragma unroll
                    for (int j = 0; j < 9; ++j) xw[(rr + 2) % 3][j] = xb[(r + 2) * LSx + j];
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                        for (int j = 0; j < 9; ++j)
#pragma unroll
                            for (int co = 0; co < 3; ++co)
                                wacc[(dy * 9 + j) * 3 + co] = fmaf(xw[(rr + dy) % 3][j], dzv[co], wacc[(dy * 9 + j) * 3 + co]);
#pragma unroll
                    for (int co = 0; co < 3; ++co) wacc[81 + co] += dzv[co];
                }
                }
            }
        } else {
        // ---- weight gradient: K = pixel groups (4 per MFMA); every wave takes rows ty = wave, wave + 4
#pragma unroll 1
        for (int ty = (DBG_FLAGS(p) & 2) ? TH : wave; ty < TH; ty += NW) {
            const int goff = n < Nw ? GOFF + (ty + 1) * LSg + TGg::HL + q * Nw + n : CST0;
            const int gstep = n < Nw ? 4 * Nw : 0;
            int aoffs[NSRC][MT];
#pragma unroll
            for (int s = 0; s < NSRC; ++s)
#pragma unroll
                for (int t = 0; t < MT; ++t)
                    aoffs[s][t] = stepA[t] ? XOFF + s * (TGx::N4 * 4) + ty * LSx + offA[t] : offA[t];
#pragma unroll
            for (int st = 0; st < TW / (4 * Gw); ++st) {
                const float bv = ldsf[goff + st * gstep];
#pragma unroll
                for (int s = 0; s < NSRC; ++s)
#pragma unroll
                    for (int t = 0; t < MT; ++t) {
                        // tiles whose 16 rows are all window rows use a compile-time step (immediate LDS offsets)
                        const int ao = 16 * (t + 1) <= 3 * WRw ? aoffs[s][t] + st * (4 * Gw * C) : aoffs[s][t] + st * stepA[t];
                        acc[s][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ldsf[ao], bv, acc[s][t], 0, 0, 0);
                    }
            }
        }
        }
        STAMP(4);
        lds_barrier();      // (barrier 2 of 2 per tile: every copy of this loop executes it, whatever its ROLE)
        STAMP(5);
        ++it;
        tile = next;
    }
