// kws_nn_int8_generic.h -- kws_nn_kernel<MAXW, TRUNK, SD>, the generic int8 network kernel.  Included once by kws_nn_int8.hip.  One template gives every
// form (include/kws/kws.h names them by label; the device symbols are the instantiations):
//   TRUNK false  the whole graph: conv blocks and head -> scores.  handoff, ci0, ci1 are not read
//   TRUNK true   the form in front of a dense stack -- no head: the last block's output of list entries ci0 .. ci1 - 1 goes to handoff [ci - ci0][fc_in]
//                in HBM, where kws_dense_i8_kernel reads it.  scores is not read
//   SD           the strided / dilated forms: output t, tap j of a block reads image row t * stride + j * dilation, image rows are counted
//                by nn_rows_sd, and a strided or dilated depthwise block takes the one-output-per-lane path.  Without SD the steps are the constant 1
//                and the rows nn_rows's: the stride-1 forms hold no test of k.stride or k.dilation.
// The argument list is shared; what `if constexpr` leaves out of an instantiation is not in its code.
// MAXW: waves per workgroup the build allows.  16 (four per SIMD) caps the kernel at 128 VGPRs, which it overruns by 20 (176 B of
// scratch per lane); 12 (three per SIMD) gives it 168 and no scratch -- the launcher picks by measurement (below).
template <int MAXW, bool TRUNK, bool SD>
__global__ __launch_bounds__(KWS_WAVE * MAXW) void kws_nn_kernel(KwsNnPlan N, const int8_t *__restrict__ q_in, int n_clips, float *__restrict__ scores,
                                                                 int8_t *__restrict__ handoff, int ci0, int ci1, NnTaps taps)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    auto rows_of = [](const KwsConvBlock &k) { if constexpr (SD) return nn_rows_sd(k); else return nn_rows(k); };      // rows of a block's input image
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), n_waves = blockDim.x >> 6;

    // ---- shared: weights, ADD tables and requantisation constants of every block, in block order ---------------
    const int fcw_bytes = nn_head_fcw_bytes(N), fcx_bytes = nn_fcx_bytes(N);
    NnHeadTab head = { nullptr, nullptr, nullptr, nullptr };
    if constexpr (!TRUNK) head = nn_head_stage(N, smem_raw, fcw_bytes);
    unsigned char *const blocks_base = smem_raw + fcw_bytes + ((KWS_HEAD_REST + 15) & ~15);
    unsigned char *sp = blocks_base;
    int act_b[2] = { 0, 0 };                           // block b reads buffer b & 1: each is sized for its own blocks
    for (int b = 0; b < N.n_blocks; ++b) {
        const KwsConvBlock &k = N.blk[b];
        const int wbytes = k.w_bytes;
        for (int i = threadIdx.x * 4; i < wbytes; i += blockDim.x * 4) *(int *)(sp + i) = *(const int *)(k.w + i);
        sp += (wbytes + 15) & ~15;
        const int lbytes = k.has_lut ? k.out_c * 256 : 0;
        for (int i = threadIdx.x * 4; i < lbytes; i += blockDim.x * 4) *(int *)(sp + i) = *(const int *)(k.add_lut + i);
        sp += lbytes;
        for (int i = threadIdx.x; i < k.out_c; i += blockDim.x) ((int4 *)sp)[i] = make_int4(k.bias_eff[i], k.mult[i], k.shift[i], 0);
        sp += k.out_c * 16;
        const int ab = rows_of(k) * k.in_cpad;
        act_b[b & 1] = max(act_b[b & 1], ab);
    }
    act_b[0] = (act_b[0] + 15) & ~15; act_b[1] = (act_b[1] + 15) & ~15;
    // per wave: two activation buffers (ping-pong) + a small vector for FC/softmax
    int8_t *actA = (int8_t *)(sp + wave * (act_b[0] + act_b[1] + fcx_bytes + 64 * 4));
    int8_t *actB = actA + act_b[0];
    int8_t *fcx = actB + act_b[1];                    // the FULLY_CONNECTED input vector (last block's pooled output)
    int *lgv = (int *)(fcx + fcx_bytes);               // logits; until the head runs, the sink of stores that fall outside the image
    int8_t *const sink = (int8_t *)lgv + 4 * lane;
    __syncthreads();

    const int F = N.n_features;
    // i / in_c for i < n_features <= 4096 as a multiply + shift (exact: i * 1 < 2^20 / in_c for in_c <= 64)
    const unsigned inv_c = (1u << 20) / (unsigned)N.blk[0].in_c + 1u;
    const bool profiling = taps.prof != nullptr && blockIdx.x == 0 && wave == 0;
    long long ph[KWS_MAX_BLOCKS + 2] = { 0 }, tlast = profiling ? clock64() : 0;
    auto mark = [&](int i) { if (profiling) { const long long now = clock64(); ph[i] += now - tlast; tlast = now; } };
    const int n_sel = TRUNK ? min(sel_count(taps.sel, n_clips), ci1) : sel_count(taps.sel, n_clips);
    for (int ci = (TRUNK ? ci0 : 0) + blockIdx.x * n_waves + wave; ci < n_sel; ci += gridDim.x * n_waves) {
        const int clip = sel_clip(taps.sel, ci);
        // ---- stage the int8 input as [pad_left + t][in_cpad], padding = zero point ((x + offset) == 0) -------
        {
            const KwsConvBlock &k = N.blk[0];
            const int rows = rows_of(k);
            const int zp4 = (int)((unsigned)(k.in_zp & 0xff) * 0x01010101u);
            for (int i = lane * 16; i < rows * k.in_cpad; i += 64 * 16) *(int4 *)(actA + i) = make_int4(zp4, zp4, zp4, zp4);
            WAVE_SYNC();
            const int8_t *src = q_in + (size_t)clip * F;
            if ((k.in_c & 3) == 0) {                       // four channels per copy (feature vector and rows 4-byte aligned)
                for (int i = lane * 4; i < k.in_w * k.in_c; i += 64 * 4) {
                    const int tt = (int)(((unsigned)i * inv_c) >> 20), c = i - tt * k.in_c;
                    *(int *)(actA + (tt + k.pad_left) * k.in_cpad + c) = *(const int *)(src + i);
                }
            } else {
                for (int i = lane; i < k.in_w * k.in_c; i += 64) {
                    const int tt = (int)(((unsigned)i * inv_c) >> 20), c = i - tt * k.in_c;       // i / in_c
                    actA[(tt + k.pad_left) * k.in_cpad + c] = src[i];
                }
            }
            WAVE_SYNC();
        }
        mark(0);
        int8_t *cur = actA, *nxt = actB;
        int pooled_off = 0;
        const unsigned char *bp = blocks_base;
        for (int b = 0; b < N.n_blocks; ++b) {
            const KwsConvBlock &k = N.blk[b];
            // this block's share of the workgroup's LDS block (kept as running pointers: an array of them would be indexed
            // through the scalar unit per access)
            const int8_t *wb = (const int8_t *)bp;
            bp += (k.w_bytes + 15) & ~15;
            const int8_t *lutb = (const int8_t *)bp;
            bp += k.has_lut ? k.out_c * 256 : 0;
            const int4 *rqt = (const int4 *)bp;
            bp += k.out_c * 16;
            const bool last = (b + 1 == N.n_blocks);
            const int nrows = last ? 0 : rows_of(N.blk[b + 1]);
            const int ncp = last ? k.out_c : N.blk[b + 1].in_cpad;
            const int npl = last ? 0 : N.blk[b + 1].pad_left;
            if (!last) {
                const int zp4 = (int)((unsigned)(N.blk[b + 1].in_zp & 0xff) * 0x01010101u);
                for (int i = lane * 16; i < nrows * ncp; i += 64 * 16) *(int4 *)(nxt + i) = make_int4(zp4, zp4, zp4, zp4);
                WAVE_SYNC();
            }
            const int out_c = k.out_c, out_w = k.out_w, n_out = k.pool_w * out_c;
            const int out_zp = k.out_zp, act_min = k.act_min, act_max = k.act_max;
            const bool has_lut = k.has_lut != 0;
            // output (pooled row pw, channel oc) lands at dbase + pw * dstride + oc; the optional debug tap mirrors it in HBM
            int8_t *const dbase = last ? fcx : nxt + npl * ncp;
            const int dstride = last ? out_c : ncp;
            int8_t *const tp = taps.pooled ? taps.pooled + (size_t)clip * taps.pooled_stride + pooled_off : nullptr;
            // one accumulator at a time (the paths below that are not worth batching)
            auto finish = [&](int m, int pw, int oc, const NnRq &q) {
                const int r = nn_requant(m, q, out_zp, act_min, act_max);
                const int8_t o = has_lut ? lutb[oc * 256 + (r + 128)] : (int8_t)r;
                dbase[pw * dstride + oc] = o;
                if (tp) tp[pw * out_c + oc] = o;
            };
            const int cs = SD ? k.stride : 1, cd = SD ? k.dilation : 1;      // image rows between two consecutive outputs / taps
            // the 4-channel depthwise path's row registers are sized at compile time for contiguous rows: a strided or dilated depthwise block takes the
            // one-output-per-lane path below (a register window of (tb - 1) * stride + (taps - 1) * dilation + 1 rows has no bound the compiler could unroll to)
            if (k.depthwise && k.depth_mult == 1 && (out_c & 3) == 0 && k.taps <= 8 && cs == 1 && cd == 1) {
                // integer_ops/depthwise_conv.h:64-103, one input channel per output.  A lane owns 4 consecutive channels of
                // one pooling window (or of 8 time steps when the block is not pooled): the tb + taps - 1 activation rows
                // it needs are read ONCE as 32-bit words (4 channels each), the 4 x taps weights as 8 words, everything
                // else is register arithmetic.  Outputs are requantised as a batch, looked up as a batch and stored four
                // channels per word.
                const bool pooled = k.pool > 1;
                const int tb = pooled ? k.pool : KWS_POOL_MAX, tstride = pooled ? k.pool_stride : KWS_POOL_MAX;
                const int n_tb = pooled ? k.pool_w : (out_w + KWS_POOL_MAX - 1) / KWS_POOL_MAX;
                const int n_cg = out_c >> 2, tp4 = (k.taps + 3) & ~3, nrow = tb + k.taps - 1;
                for (int item = lane; item < n_tb * n_cg; item += 64) {
                    const int pw = item / n_cg, oc0 = (item - pw * n_cg) * 4;
                    const int t0 = pw * tstride;
                    int xw[KWS_POOL_MAX + 7], ww[4][2];
#pragma unroll
                    for (int r = 0; r < KWS_POOL_MAX + 7; ++r)
                        xw[r] = r < nrow ? *(const int *)(cur + (t0 + r) * k.in_cpad + oc0) : 0;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int *wr = (const int *)(wb + (oc0 + c) * tp4);
                        ww[c][0] = wr[0];
                        ww[c][1] = tp4 > 4 ? wr[1] : 0;
                    }
                    NnRq rq[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) rq[c] = nn_rq_of(rqt, oc0 + c);
                    int acc[KWS_POOL_MAX][4];
#pragma unroll
                    for (int i = 0; i < KWS_POOL_MAX; ++i)
#pragma unroll
                        for (int c = 0; c < 4; ++c) acc[i][c] = 0;
#pragma unroll
                    for (int tap = 0; tap < 8; ++tap) {
                        if (tap < k.taps) {
#pragma unroll
                            for (int c = 0; c < 4; ++c) {
                                const int wv = (ww[c][tap >> 2] << (24 - 8 * (tap & 3))) >> 24;      // sign-extended byte
#pragma unroll
                                for (int i = 0; i < KWS_POOL_MAX; ++i)
                                    if (i < tb) acc[i][c] += wv * ((xw[i + tap] << (24 - 8 * c)) >> 24);
                            }
                        }
                    }
                    if (pooled) {
                        int o[4];
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            int m = (int)0x80000000;
#pragma unroll
                            for (int i = 0; i < KWS_POOL_MAX; ++i)
                                if (i < tb && t0 + i < out_w) m = max(m, acc[i][c]);
                            o[c] = nn_requant(m, rq[c], out_zp, act_min, act_max);
                        }
                        if (has_lut)
#pragma unroll
                            for (int c = 0; c < 4; ++c) o[c] = lutb[(oc0 + c) * 256 + (o[c] + 128)];
                        const int word = (o[0] & 0xff) | ((o[1] & 0xff) << 8) | ((o[2] & 0xff) << 16) | ((int)((unsigned)o[3] << 24));
                        *(int *)(dbase + pw * dstride + oc0) = word;
                        if (tp)
#pragma unroll
                            for (int c = 0; c < 4; ++c) tp[pw * out_c + oc0 + c] = (int8_t)o[c];
                    } else {
#pragma unroll
                        for (int i = 0; i < KWS_POOL_MAX; ++i) {               // a time step's four channels: one word
                            int o[4];
#pragma unroll
                            for (int c = 0; c < 4; ++c) o[c] = nn_requant(acc[i][c], rq[c], out_zp, act_min, act_max);
                            if (has_lut)
#pragma unroll
                                for (int c = 0; c < 4; ++c) o[c] = lutb[(oc0 + c) * 256 + (o[c] + 128)];
                            const int word = (o[0] & 0xff) | ((o[1] & 0xff) << 8) | ((o[2] & 0xff) << 16) | ((int)((unsigned)o[3] << 24));
                            const bool ok = t0 + i < out_w;
                            *(int *)(ok ? dbase + (t0 + i) * dstride + oc0 : sink) = word;
                            if (tp && ok)
#pragma unroll
                                for (int c = 0; c < 4; ++c) tp[(t0 + i) * out_c + oc0 + c] = (int8_t)o[c];
                        }
                    }
                }
            } else if (k.depthwise) {                    // any depth multiplier / channel count: one output per lane and pass
                const int tp4 = (k.taps + 3) & ~3;
                for (int idx = lane; idx < n_out; idx += 64) {
                    const int pw = idx / out_c, oc = idx - pw * out_c;
                    const int t0 = pw * k.pool_stride;
                    int acc[KWS_POOL_MAX];
#pragma unroll
                    for (int i = 0; i < KWS_POOL_MAX; ++i) acc[i] = 0;
                    const int8_t *wrow = wb + oc * tp4;
                    const int8_t *xcol = cur + t0 * cs * k.in_cpad + oc / k.depth_mult;
                    for (int tap = 0; tap < k.taps; ++tap) {
                        const int wv = wrow[tap];
#pragma unroll
                        for (int i = 0; i < KWS_POOL_MAX; ++i)
                            if (i < k.pool) acc[i] += wv * (int)xcol[(i * cs + tap * cd) * k.in_cpad];
                    }
                    int m = (int)0x80000000;
#pragma unroll
                    for (int i = 0; i < KWS_POOL_MAX; ++i)
                        if (i < k.pool && t0 + i < out_w) m = max(m, acc[i]);
                    finish(m, pw, oc, nn_rq_of(rqt, oc));
                }
            } else if (k.mfma) {
                // CONV_2D without pooling on v_mfma_i32_32x32x32_i8: [time x (taps * in_cpad)] x [(taps * in_cpad) x out_c], one or
                // two 32-row tiles, k-steps of 32 bytes = two taps (16-byte rows), one tap (32) or half a tap (64).  A and B use
                // the same slot -> (tap, channel) map; int32 accumulation is exact, so the sums equal the reference's scalar loops
                const int cp = k.in_cpad, n = lane & 31, hh = lane >> 5;
                const int ks = cp == 16 ? (k.taps + 1) >> 1 : cp == 32 ? k.taps : 2 * k.taps;
                const bool two = out_w > 32;
                const int nc = min(n, out_c - 1);                                              // columns >= out_c: never stored
                v16i acc0 = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 }, acc1 = acc0;
                const int8_t *wrow = wb + (size_t)nc * k.taps * cp;
                const NnRq rq = nn_rq_of(rqt, nc);
                for (int s_ = 0; s_ < ks; ++s_) {
                    const int tap = cp == 16 ? 2 * s_ + hh : cp == 32 ? s_ : s_ >> 1;
                    const int ch = cp == 16 ? 0 : cp == 32 ? 16 * hh : 32 * (s_ & 1) + 16 * hh;
                    v4i wv = { 0, 0, 0, 0 };
                    if (tap < k.taps) wv = *(const v4i *)(wrow + tap * cp + ch);
                    const v4i a0 = *(const v4i *)(cur + (n + tap) * cp + ch);                  // row = time (lane & 31) + tap
                    acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, wv, acc0, 0, 0, 0);
                    if (two) {
                        const v4i a1 = *(const v4i *)(cur + (32 + n + tap) * cp + ch);
                        acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, wv, acc1, 0, 0, 0);
                    }
                }
                // accumulator register r of a tile holds row (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), column lane & 31: the lane
                // requantises its column's 16 (32) values as a batch, looks them up as a batch, then stores (rows / columns
                // outside the image go to the sink: no branch per value)
                const int8_t *lp = lutb + nc * 256 + 128;
                int8_t *const dcol = dbase + n;
                const bool col_ok = n < out_c;
                for (int tile = 0; tile < (two ? 2 : 1); ++tile) {
                    const v16i &acc = tile ? acc1 : acc0;
                    // registers 4 g .. 4 g + 3 hold rows 32 tile + 8 g + 4 hh + 0 .. 3: a group past the image is skipped whole
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        if (32 * tile + 8 * g >= out_w) break;
                        int o[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) o[i] = nn_requant(acc[4 * g + i], rq, out_zp, act_min, act_max);
                        if (has_lut)
#pragma unroll
                            for (int i = 0; i < 4; ++i) o[i] = lp[o[i]];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int row = 32 * tile + 8 * g + 4 * hh + i;
                            const bool ok = col_ok && row < out_w;
                            *(ok ? dcol + row * dstride : sink) = (int8_t)o[i];
                            if (tp && ok) tp[row * out_c + n] = (int8_t)o[i];
                        }
                    }
                }
            } else {
                // a lane owns one pooling window of OB = 2 (or 1) output channels: every 16-byte activation read feeds
                // 4 * OB dot products, every 16-byte weight read `pool` of them
                // (an un-pooled block is walked in groups of KWS_POOL_MAX time steps, each stored on its own)
                const bool pooled = k.pool > 1;
                const int tb = pooled ? k.pool : KWS_POOL_MAX, tstride = pooled ? k.pool_stride : KWS_POOL_MAX;
                const int n_tb = pooled ? k.pool_w : (out_w + KWS_POOL_MAX - 1) / KWS_POOL_MAX;
                const int ob = (n_tb * out_c > 64 && (out_c & 1) == 0) ? 2 : 1;
                const int n_ocb = out_c / ob;
                const int c16n = k.in_cpad >> 4;
                for (int item = lane; item < n_tb * n_ocb; item += 64) {
                    const int pw = item / n_ocb, oc0 = (item - pw * n_ocb) * ob;
                    const int t0 = pw * tstride;
                    int acc[KWS_POOL_MAX][2];
#pragma unroll
                    for (int i = 0; i < KWS_POOL_MAX; ++i) acc[i][0] = acc[i][1] = 0;
                    const int8_t *w0 = wb + (size_t)oc0 * k.taps * k.in_cpad;
                    const int8_t *w1 = w0 + (ob == 2 ? k.taps * k.in_cpad : 0);
                    for (int tap = 0; tap < k.taps; ++tap) {
                        const int8_t *xrow = cur + (t0 * cs + tap * cd) * k.in_cpad;
                        const int xstep = cs * k.in_cpad;                                  // bytes between the rows of two consecutive outputs
                        for (int c16 = 0; c16 < c16n; ++c16) {
                            const int4 wa = *(const int4 *)(w0 + tap * k.in_cpad + 16 * c16);
                            const int4 wb4 = *(const int4 *)(w1 + tap * k.in_cpad + 16 * c16);
#pragma unroll
                            for (int i = 0; i < KWS_POOL_MAX; ++i) {
                                if (i < tb) {
                                    const int4 xv = *(const int4 *)(xrow + i * xstep + 16 * c16);
                                    int a = acc[i][0], c = acc[i][1];
                                    a = __builtin_amdgcn_sdot4(wa.x, xv.x, a, false);
                                    a = __builtin_amdgcn_sdot4(wa.y, xv.y, a, false);
                                    a = __builtin_amdgcn_sdot4(wa.z, xv.z, a, false);
                                    a = __builtin_amdgcn_sdot4(wa.w, xv.w, a, false);
                                    if (ob == 2) {
                                        c = __builtin_amdgcn_sdot4(wb4.x, xv.x, c, false);
                                        c = __builtin_amdgcn_sdot4(wb4.y, xv.y, c, false);
                                        c = __builtin_amdgcn_sdot4(wb4.z, xv.z, c, false);
                                        c = __builtin_amdgcn_sdot4(wb4.w, xv.w, c, false);
                                    }
                                    acc[i][0] = a; acc[i][1] = c;
                                }
                            }
                        }
                    }
                    for (int o = 0; o < ob; ++o) {
                        const NnRq rq = nn_rq_of(rqt, oc0 + o);
                        if (pooled) {
                            int m = (int)0x80000000;
#pragma unroll
                            for (int i = 0; i < KWS_POOL_MAX; ++i)
                                if (i < tb && t0 + i < out_w) m = max(m, acc[i][o]);
                            finish(m, pw, oc0 + o, rq);
                        } else {
#pragma unroll
                            for (int i = 0; i < KWS_POOL_MAX; ++i)
                                if (t0 + i < out_w) finish(acc[i][o], t0 + i, oc0 + o, rq);
                        }
                    }
                }
            }
            pooled_off += n_out;
            WAVE_SYNC();
            mark(1 + b);
            int8_t *tmp = cur; cur = nxt; nxt = tmp;
        }
        if constexpr (TRUNK) {
            int8_t *dst = handoff + (size_t)(ci - ci0) * N.fc_in;
            for (int i = lane; i < N.fc_in; i += 64) dst[i] = fcx[i];
            WAVE_SYNC();
        } else nn_head(N, head, fcx, lgv, lane, clip, scores, taps);
        mark(1 + KWS_MAX_BLOCKS);
    }
    if (profiling && lane == 0)
        for (int i = 0; i < KWS_MAX_BLOCKS + 2; ++i) taps.prof[i] = ph[i];
}
