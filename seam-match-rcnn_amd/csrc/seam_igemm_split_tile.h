// seam_igemm_split_tile.h -- the tile program of the split-bf16 implicit-GEMM kernels, conv_igemm_bx3 and conv_igemm_sx
// (seam_conv.hip), written once.  NOT a stand-alone header: it is the statements of a kernel body, included inside each of the two
// kernels with these names in scope:
//   p            the kernel's ConvArgs
//   Form         FormBx3 or FormSx<TERMS> (seam_conv.hip): planes per operand, the cut of an A vector, the packed weight
//                layout, the term table, and whether the tile ends with the 16-byte epilogue
//   BM, BN, NW   block tile and waves per block
// Pipeline: the fp32 kernel's gather (raw buffer loads, the (r, c-chunk, s) chunk walk, hardware zero fill), a ring of two register
// sets, the cut of A at the LDS store, two LDS buffers of XOR-swizzled 64-byte rows, one plane per piece, and per chunk two k-steps
// of Form::TERMS * MT * NT MFMAs with the loads behind the first and the LDS stores and the barrier behind the second.
    constexpr int ES = 4, EPV = 4, BKE = 32;
    constexpr int PLANES = Form::PLANES;
    constexpr int WM = BM / (NW / 2), WN = BN / 2;
    constexpr int MT = WM / 32, NT = WN / 32;
    constexpr int RP = 8 * NW;
    constexpr int AI = BM / RP, BI = Form::template BI<BN, NW>;      // 16-byte loads per thread per chunk
    constexpr int Q = Form::TERMS * MT * NT;     // MFMAs per k-step (16 k-values)
    constexpr int PA = BM * 64 + 64;             // bytes of one A plane (+64: the next plane starts on the other bank half)
    constexpr int PB = BN * 64 + 64;

    __shared__ __attribute__((aligned(16))) char As[2][PLANES * PA];     // [buffer][plane 0 | 1 (| 2)]
    __shared__ __attribute__((aligned(16))) char Bs[2][PLANES * PB];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int wm0 = (wid >> 1) * WM;
    const int wn0 = (wid & 1) * WN;

    const int nblk = gridDim.x;
    const int b = blockIdx.x;
    const int xcd = b & 7;
    const int q8 = nblk >> 3, rem = nblk & 7;
    const int tile = (xcd < rem ? xcd * (q8 + 1) : rem * (q8 + 1) + (xcd - rem) * q8) + (b >> 3);
    const int tm = tile / p.tiles_n;
    const int tn = tile - tm * p.tiles_n;
    const int m0 = tm * BM;
    const int n0 = tn * BN;

    const int nk = p.kred / BKE;
    const int lcol = tid & 7;
    const int lrow = tid >> 3;
    const int HoWo = p.Ho * p.Wo;
    const int n_first = m0 / HoWo;
    const size_t img_elems = (size_t)p.H * p.W * p.C;
    const size_t rem_bytes = ((size_t)(p.N - n_first) * img_elems) * ES;
    const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)p.x + (size_t)n_first * img_elems * ES), 0,
        (int)(rem_bytes > kOob ? kOob : (unsigned)rem_bytes), 0x00020000);
    const int slab_stride = Form::chunk_stride(p);
    const int n_in_slab = n0 % p.slab_bn;
    const __amdgpu_buffer_rsrc_t b_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)Form::w_base(p, n0, n_in_slab), 0, (int)((unsigned)nk * (unsigned)slab_stride), 0x00020000);

    int arow[AI], ahi[AI], awi[AI];
#pragma unroll
    for (int i = 0; i < AI; ++i) {
        const int m = m0 + lrow + RP * i;
        if (m < p.M) {
            const int n = m / HoWo;
            const int rm = m - n * HoWo;
            const int ho = rm / p.Wo;
            const int wo = rm - ho * p.Wo;
            ahi[i] = ho * p.stride - p.pad;
            awi[i] = wo * p.stride - p.pad;
            arow[i] = ((((n - n_first) * p.H + ahi[i]) * p.W + awi[i]) * p.C) * ES;
        } else {
            ahi[i] = -(1 << 28);
            awi[i] = 0;
            arow[i] = 0;
        }
    }
    int brow[BI];
#pragma unroll
    for (int i = 0; i < BI; ++i) brow[i] = Form::template brow<BN, NW>(p, i, tid, lrow, lcol, n_in_slab);

    int kc, kr, ks, tapoff;
    {
        const int kk = lcol * EPV;
        const int pos = kk / p.C;
        kc = kk - pos * p.C;
        kr = pos / p.S;
        ks = pos - kr * p.S;
        tapoff = ((kr * p.W + ks) * p.C + kc) * ES;
    }
    int uq = 0;

    constexpr int D = 2;
    f32x4 areg[D][AI], breg[D][BI];
    auto load_a = [&](f32x4 (&ar)[AI], int i) {
        const bool ok = (unsigned)(ahi[i] + kr) < (unsigned)p.H && (unsigned)(awi[i] + ks) < (unsigned)p.W && kr < p.R;
        const unsigned off = ok ? (unsigned)(arow[i] + tapoff) : kOob;
        if (!(SEAM_BX3_ABL & 1)) ar[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, off, 0, 0));
    };
    auto load_b = [&](f32x4 (&br)[BI], int i) {
        const int so = uq < nk ? uq * slab_stride : (int)kOob;
        if (!(SEAM_BX3_ABL & 1)) br[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, brow[i], so, 0));
    };
    auto advance_k = [&]() {
        ++uq;
        if (p.C >= BKE) {
            if (++ks == p.S) {
                ks = 0;
                kc += BKE;
                if (kc >= p.C) { kc -= p.C; ++kr; }
            }
        } else {
            kc += BKE;
            while (kc >= p.C) {
                kc -= p.C;
                if (++ks == p.S) { ks = 0; ++kr; }
            }
        }
        tapoff = ((kr * p.W + ks) * p.C + kc) * ES;
    };
    auto load_chunk = [&](f32x4 (&ar)[AI], f32x4 (&br)[BI]) {
#pragma unroll
        for (int i = 0; i < AI; ++i) load_a(ar, i);
#pragma unroll
        for (int i = 0; i < BI; ++i) load_b(br, i);
        advance_k();
    };
    // LDS addresses of this thread's stores.  A: 4 floats -> 8 B in each plane at bf16 index 4*lcol of the row;
    // B: 16 B of one plane's row, where the form's weight layout puts them.
    auto store_row = [&](const f32x4 (&ar)[AI], const f32x4 (&br)[BI], int buf, int r) {
        if (SEAM_BX3_ABL & 2) return;
        if (r < AI) {
            const int row = lrow + RP * r;
            const int off = row * 64 + ((((lcol >> 1) ^ (row >> 2)) & 3) << 4) + (lcol & 1) * 8;
            u32x2 q0, q1, q2;
            if (SEAM_BX3_ABL & 4) { q0[0] = __builtin_bit_cast(unsigned, ar[r][0]); q0[1] = __builtin_bit_cast(unsigned, ar[r][1]);
                                    q1[0] = __builtin_bit_cast(unsigned, ar[r][2]); q1[1] = __builtin_bit_cast(unsigned, ar[r][3]); q2 = q0; }
            else Form::cut(ar[r], q0, q1, q2);
            *reinterpret_cast<u32x2*>(&As[buf][off]) = q0;
            *reinterpret_cast<u32x2*>(&As[buf][PA + off]) = q1;
            if constexpr (PLANES == 3) *reinterpret_cast<u32x2*>(&As[buf][2 * PA + off]) = q2;
        } else {
            // (written out per form, not a Form function: any helper tried here changed the order of this address sum in the
            //  assembly of some instance, profiles/igemm_split_fold.txt 2b)
            const int i = r - AI;
            if constexpr (PLANES == 2) {      // Form::brow's vector: lcol < 4 -> hi plane slot lcol, else lo plane slot lcol-4
                const int row = lrow + RP * i;
                const int off = (lcol >> 2) * PB + row * 64 + (((lcol ^ (row >> 2)) & 3) << 4);
                *reinterpret_cast<f32x4*>(&Bs[buf][off]) = br[i];
            } else {                          // Form::brow's vector: plane pl, row and slot of the tile's [plane][BN rows][4 slots]
                constexpr int VPP = BN * 4;
                const int pl = (64 * NW * i) / VPP, within = tid + (64 * NW * i) % VPP;
                const int row = within >> 2;
                *reinterpret_cast<f32x4*>(&Bs[buf][pl * PB + row * 64 + ((((within & 3) ^ (row >> 2)) & 3) << 4)]) = br[i];
            }
        }
    };

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // fragment addresses: lane reads 16 B (8 bf16 of k) of row (l & 31) at slot 2*step + (l >> 5), swizzled
    const int arow0 = wm0 + (lane & 31), brow0 = wn0 + (lane & 31);
    struct Frag { f32x4 a[PLANES][MT], b[PLANES][NT]; };
    Frag f0, f1;
    auto read_frags = [&](Frag& f, int buf, int step) {
        if (SEAM_BX3_ABL & 16) return;
        const int slot = 2 * step + (lane >> 5);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int row = arow0 + i * 32;
            const int off = row * 64 + (((slot ^ (row >> 2)) & 3) << 4);
#pragma unroll
            for (int pl = 0; pl < PLANES; ++pl) f.a[pl][i] = *reinterpret_cast<const f32x4*>(&As[buf][pl * PA + off]);
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int row = brow0 + j * 32;
            const int off = row * 64 + (((slot ^ (row >> 2)) & 3) << 4);
#pragma unroll
            for (int pl = 0; pl < PLANES; ++pl) f.b[pl][j] = *reinterpret_cast<const f32x4*>(&Bs[buf][pl * PB + off]);
        }
    };
    auto mf = [&](const Frag& f, int idx) {       // idx in [0, Q): term-major, the smallest terms of a tile first
        const int term = Form::term(idx / (MT * NT)), i = (idx / NT) % MT, j = idx % NT;
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, f.a[term >> 2][i]),
                                                            __builtin_bit_cast(bf16x8, f.b[term & 3][j]), acc[i][j], 0, 0, 0);
    };

    auto chunk = [&](int buf, f32x4 (&lda)[AI], f32x4 (&ldb)[BI], const f32x4 (&sta)[AI], const f32x4 (&stb)[BI]) {
        // k-step 0 (+ the gathers and weight rows of chunk t+D)
        read_frags(f1, buf, 1);
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            mf(f0, q);
#pragma unroll
            for (int i = 0; i < AI + BI; ++i)
                if ((i * Q) / (AI + BI) == q) {
                    if (i < AI) load_a(lda, i);
                    else load_b(ldb, i - AI);
                }
            if (q == Q - 1) advance_k();
        }
        // k-step 1: chunk t+1 goes to the other LDS buffer behind the first two thirds of the MFMAs, then the barrier
        // and the first fragments of the next chunk; the last third covers their latency
        constexpr int QS = (2 * Q) / 3;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            mf(f1, q);
#pragma unroll
            for (int r = 0; r < AI + BI; ++r)
                if ((r * QS) / (AI + BI) == q) store_row(sta, stb, buf ^ 1, r);
            if (q == QS - 1) {
                if (!(SEAM_BX3_ABL & 8)) __syncthreads();
                read_frags(f0, buf ^ 1, 0);
            }
        }
    };

    load_chunk(areg[0], breg[0]);
#pragma unroll
    for (int r = 0; r < AI + BI; ++r) store_row(areg[0], breg[0], 0, r);
    load_chunk(areg[1], breg[1]);
    __syncthreads();
    read_frags(f0, 0, 0);

    for (int t = 0; t < nk; t += 2) {
        chunk(0, areg[0], breg[0], areg[1], breg[1]);
        if (t + 1 < nk) chunk(1, areg[1], breg[1], areg[0], breg[0]);
    }

    if constexpr (Form::VEC_EPI) __syncthreads();     // every wave is done with the LDS buffers: the epilogue's transpose reuses them

    // ---- epilogue (the fp32 kernel's; its 16-byte form through a wave-private LDS transpose when the form asks and K % 4 == 0) ----
    const size_t tile_off = (size_t)m0 * p.K;
    const unsigned rows_here = (unsigned)min(BM, p.M - m0);
    const __amdgpu_buffer_rsrc_t y_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((char*)p.y + tile_off * 4), 0, (int)(rows_here * (unsigned)p.K * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t r_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)(p.res ? p.res : p.y) + tile_off * 4), 0, (int)(rows_here * (unsigned)p.K * 4), 0x00020000);
    if (Form::VEC_EPI && (p.K & 3) == 0) {
        constexpr int EW = WN + 4;                 // padded row, floats
        constexpr int LPR = WN / 4;                // lanes per row
        constexpr int RPI = 64 / LPR;              // rows per 16-byte pass of the wave
        constexpr int NP = 32 / RPI;               // passes per 32-row MFMA tile
        static_assert(!Form::VEC_EPI || NW * 32 * EW * 4 <= 2 * PLANES * (BM >= BN ? PA : PB), "the transpose fits the operand's LDS");
        float* eb = reinterpret_cast<float*>(BM >= BN ? &As[0][0] : &Bs[0][0]) + wid * 32 * EW;
        const int er = lane / LPR, ec = (lane % LPR) * 4;
        const int n = n0 + wn0 + ec;
        const bool nok = n < p.K;
        f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
        if (p.scale && nok) sc = *reinterpret_cast<const f32x4*>(p.scale + n);
        if (p.shift && nok) sh = *reinterpret_cast<const f32x4*>(p.shift + n);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            unsigned eo[NP];
            f32x4 rv[NP];
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const int row = wm0 + i * 32 + k * RPI + er;
                eo[k] = nok ? (unsigned)(row * p.K + n) * 4u : kOob;
            }
            if (p.res) {
#pragma unroll
                for (int k = 0; k < NP; ++k)
                    rv[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_rsrc, eo[k], 0, 0));
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    eb[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * EW + j * 32 + (lane & 31)] = acc[i][j][r];
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                f32x4 v = *reinterpret_cast<const f32x4*>(&eb[(k * RPI + er) * EW + ec]) * sc + sh;
                if (p.res) {
                    if (p.relu == 2) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = rv[k][e] > 0.f ? v[e] : 0.f;
                    } else {
                        v += rv[k];
                    }
                }
                if (p.relu == 1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                }
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), y_rsrc, eo[k], 0, 0);
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = n0 + wn0 + j * 32 + (lane & 31);
        const bool nok = n < p.K;
        const float sc = (p.scale && nok) ? p.scale[n] : 1.f;
        const float sh = (p.shift && nok) ? p.shift[n] : 0.f;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            unsigned eo[16];
            float rv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                eo[r] = (unsigned)(row * p.K + n);
            }
            if (p.res) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    rv[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r_rsrc, nok ? eo[r] * 4u : kOob, 0, 0));
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = acc[i][j][r] * sc + sh;
                if (p.res) v = p.relu == 2 ? (rv[r] > 0.f ? v : 0.f) : v + rv[r];
                if (p.relu == 1) v = fmaxf(v, 0.f);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), y_rsrc, nok ? eo[r] * 4u : kOob, 0, 0);
            }
        }
    }
