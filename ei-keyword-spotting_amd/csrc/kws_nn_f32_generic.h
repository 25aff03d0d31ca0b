// kws_nn_f32_generic.h -- kws_nn_f32_kernel<MAXT, TRUNK, SD>, the generic float32 network kernel.  Included once by kws_nn_f32.hip, after the helpers it
// calls.  One template gives every form (include/kws/kws.h names them by label; the device symbols are the instantiations):
//   TRUNK false  the whole graph: conv blocks, FULLY_CONNECTED, SOFTMAX -> scores (tap_logits: the optional logit tap).  handoff, ci0, ci1 are not read
//   TRUNK true   the form in front of a dense stack -- no head: the last block's output of list entries ci0 .. ci1 - 1 goes to handoff [ci - ci0][fc_in]
//                in HBM, where kws_dense_f32_kernel reads it.  scores and tap_logits are not read
//   SD           the strided / dilated forms: every block's convolution goes through nnf_conv_ob_sd
// The argument list is shared; what `if constexpr` leaves out of an instantiation is not in its code.
template <int MAXT, bool TRUNK, bool SD>     // MAXT: threads per workgroup the build allows: 1024 (<= 128 VGPRs) or 512 (<= 256 VGPRs, vectorised conv steps)
__global__ __launch_bounds__(MAXT) void kws_nn_f32_kernel(const KwsNnPlanF32 *__restrict__ Np, const float *__restrict__ features, int n_clips,
                                                          float *__restrict__ scores, float *__restrict__ tap_logits, float *__restrict__ handoff, int ci0,
                                                          int ci1, long long *__restrict__ prof, const int *__restrict__ sel)
{
    // the plan is read from memory (scalar loads, any block index); by value in the kernel arguments the compiler copies it to
    // scratch as soon as a block is indexed dynamically
    const KwsNnPlanF32 &N = *Np;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), n_waves = blockDim.x >> 6;
    // development aid: shader-clock totals per phase of wave 0 of workgroup 0 (input, each block, head)
    const bool profiling = prof != nullptr && blockIdx.x == 0 && wave == 0;
    long long ph[KWS_MAX_BLOCKS + 2] = { 0 }, tlast = profiling ? clock64() : 0;
    auto mark = [&](int i) { if (profiling) { const long long now = clock64(); ph[i] += now - tlast; tlast = now; } };
    // a workgroup none of whose waves has a clip (the empty re-run list of a KWS_MODE_FAST call, a short list) leaves before
    // the weights are staged: 16.5 us -> launch overhead for the empty list
    const int first = TRUNK ? ci0 : 0;               // the list entry of workgroup 0, wave 0
    const int n_sel = TRUNK ? min(sel_count(sel, n_clips), ci1) : sel_count(sel, n_clips);
    if (first + (int)blockIdx.x * n_waves >= n_sel) return;
    float *sp = (float *)smem_raw;
    int s_w_off[KWS_MAX_BLOCKS];     // float offsets into the LDS block: pointers kept in an array lose their address space (flat loads)
    for (int b = 0; b < N.n_blocks; ++b) {
        const KwsConvBlockF32 &k = N.blk[b];
        const int J = k.depthwise ? k.taps : k.taps * k.in_c, ocp = nnf_ocp(k);
        for (int i = threadIdx.x; i < J * ocp; i += blockDim.x) {      // [oc][j] -> [j][oc], zero in the padding channels
            const int j = i / ocp, oc = i - j * ocp;
            sp[nnf_w_index(k, J, j, oc)] = oc < k.out_c ? (k.depthwise ? k.w[j * k.out_c + oc] : k.w[oc * J + j]) : 0.0f;
        }
        s_w_off[b] = (int)(sp - (float *)smem_raw);
        sp += J * ocp;
    }
    const NnfLayout L = nnf_layout(N);
    const float *s_fcw = sp, *s_fcb = sp + N.fc_out * N.fc_in;
    if constexpr (!TRUNK) {
        for (int i = threadIdx.x; i < N.fc_out * N.fc_in; i += blockDim.x) sp[i] = N.fc_w[i];
        for (int i = threadIdx.x; i < N.fc_out; i += blockDim.x) sp[N.fc_out * N.fc_in + i] = N.fc_bias[i];
    }
    sp += L.fc_floats;
    float *A = sp + wave * (L.a_floats + L.b_floats + L.y_floats + L.vec_floats);
    float *B = A + L.a_floats;
    float *Y = B + L.b_floats;
    float *vec = Y + L.y_floats;
    __syncthreads();

    // next-clip prefetch registers (256-register build only): NNF_PF x 64 float4 cover the first block's padded input image
    constexpr int NNF_PF = 9;
    float4 pf[NNF_PF];
#pragma unroll
    for (int u = 0; u < NNF_PF; ++u) pf[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    bool have_pf = false;
    const bool pf_ok = [&]() {
        const KwsConvBlockF32 &k = N.blk[0];
        const int lo = k.pad_left * k.in_c, hi = lo + k.in_w * k.in_c, tot = nnf_rows(k) * k.in_c;
        return ((lo | hi | N.n_features) & 3) == 0 && ((tot + 3) >> 2) <= 64 * NNF_PF && N.n_blocks > 1;
    }();
    for (int ci = first + blockIdx.x * n_waves + wave; ci < n_sel; ci += gridDim.x * n_waves) {
        const int clip = sel_clip(sel, ci);
        {
            const KwsConvBlockF32 &k = N.blk[0];
            const int lo = k.pad_left * k.in_c, hi = lo + k.in_w * k.in_c, tot = nnf_rows(k) * k.in_c;
            const float *src = features + (size_t)clip * N.n_features;
            if (have_pf) {
                // the feature vector was requested while the previous clip's tail blocks ran (see below): it only has to be
                // placed, zero padding rows included
                float4 *A4 = (float4 *)A;
                const int lo4 = lo >> 2, hi4 = hi >> 2, tot4 = (tot + 3) >> 2;
#pragma unroll
                for (int u = 0; u < NNF_PF; ++u) {
                    const int i = lane + 64 * u;
                    if (i < tot4) A4[i] = (i >= lo4 && i < hi4) ? pf[u] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            } else if (((lo | hi | N.n_features) & 3) == 0) {
                // 16-byte copies (the feature vector of a clip and its place in the image are both 16-byte aligned)
                const float4 *src4 = (const float4 *)src;
                float4 *A4 = (float4 *)A;
                const int lo4 = lo >> 2, hi4 = hi >> 2, tot4 = (tot + 3) >> 2;
                for (int i0 = lane; i0 < tot4; i0 += 64 * 4) {
                    float4 v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int i = i0 + 64 * u;
                        v[u] = (i >= lo4 && i < hi4) ? src4[i - lo4] : make_float4(0.f, 0.f, 0.f, 0.f);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int i = i0 + 64 * u;
                        if (i < tot4) A4[i] = v[u];
                    }
                }
            } else {
                // 8 loads per lane in flight (one at a time this stage is a chain of global-memory round trips)
                for (int i0 = lane; i0 < tot; i0 += 64 * 8) {
                    float v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int i = i0 + 64 * u;
                        v[u] = (i >= lo && i < hi) ? src[i - lo] : 0.0f;
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int i = i0 + 64 * u;
                        if (i < tot) A[i] = v[u];
                    }
                }
            }
            WAVE_SYNC();
        }
        mark(0);
        for (int b = 0; b < N.n_blocks; ++b) {
            // a COPY of the block's parameters (scalar registers): through the reference every epilogue step reloads its clamp
            // bounds and strides from memory, because the LDS stores in between might alias the plan
            const KwsConvBlockF32 k = N.blk[b];
            const bool last = (b + 1 == N.n_blocks);
            const float *cur = (b & 1) ? B : A;
            NnfDst dst;
            const int n_out = k.pool_w * k.out_c;
            if (last) { dst.p = vec; dst.row0 = 0; dst.stride = k.out_c; }
            else {
                const KwsConvBlockF32 &nk = N.blk[b + 1];
                dst.p = (b & 1) ? A : B; dst.row0 = nk.pad_left; dst.stride = nk.in_c;
                // the zero padding rows of the next block's input image (its real rows are written below)
                const int lo = nk.pad_left * nk.in_c, hi = lo + n_out, tot = nnf_rows(nk) * nk.in_c;
                for (int i = lane; i < tot; i += 64)
                    if (i < lo || i >= hi) dst.p[i] = 0.0f;
            }
            const float *wt = (const float *)smem_raw + s_w_off[b];
            switch (k.tb) {
            case 8: nnf_conv_ob<8, (MAXT <= 512), SD>(k, cur, wt, Y, dst, lane); break;
            case 7: nnf_conv_ob<7, (MAXT <= 512), SD>(k, cur, wt, Y, dst, lane); break;
            case 4: nnf_conv_ob<4, (MAXT <= 512), SD>(k, cur, wt, Y, dst, lane); break;
            case 2: nnf_conv_ob<2, (MAXT <= 512), SD>(k, cur, wt, Y, dst, lane); break;
            default: nnf_conv_ob<1, (MAXT <= 512), SD>(k, cur, wt, Y, dst, lane); break;
            }
            WAVE_SYNC();
            if (b == 0 && MAXT <= 512 && pf_ok) {
                // block 0 (most of the clip's time) is done: request the NEXT clip's feature vector now, so that it arrives
                // while the short tail blocks, FC and softmax run (phases with little VALU work and nothing to prefetch)
                const int nci = ci + gridDim.x * n_waves;
                have_pf = nci < n_sel;
                if (have_pf) {
                    const int nclip = sel_clip(sel, nci);
                    const KwsConvBlockF32 &k0 = N.blk[0];
                    const int lo4 = (k0.pad_left * k0.in_c) >> 2, hi4 = lo4 + ((k0.in_w * k0.in_c) >> 2);
                    const float4 *src4 = (const float4 *)(features + (size_t)nclip * N.n_features);
#pragma unroll
                    for (int u = 0; u < NNF_PF; ++u) {
                        const int i = lane + 64 * u;
                        if (i >= lo4 && i < hi4) pf[u] = src4[i - lo4];
                    }
                }
            }
            if (nnf_staged(k)) {
                // MAX_POOL_2D over time (pooling.h:189-237) from the staged conv output
                for (int idx = lane; idx < n_out; idx += 64) {
                    const int pw = nnf_div(idx, k.out_c, k.inv_outc20), oc = idx - pw * k.out_c;
                    float mx = -FLT_MAX;
                    for (int q = 0; q < k.pool && pw * k.pool_stride + q < k.out_w; ++q) {      // the last window may be ragged (SAME)
                        const float v = Y[(pw * k.pool_stride + q) * k.out_c + oc];
                        mx = mx < v ? v : mx;                          // std::max(max, v)
                    }
                    dst.p[(dst.row0 + pw) * dst.stride + oc] = act_clamp(mx, k.pool_min, k.pool_max);
                }
                WAVE_SYNC();
            }
            mark(1 + b);
        }
        if constexpr (TRUNK) {
            float *dst = handoff + (size_t)(ci - ci0) * N.fc_in;
            for (int i = lane; i < N.fc_in; i += 64) dst[i] = vec[i];
            WAVE_SYNC();
        } else {
            // FULLY_CONNECTED (fully_connected.h:26-60) + SOFTMAX (softmax.h:31-63)
            float *lg = vec + (L.vec_floats - 64), *ex = vec;          // ex overwrites the FC input once every lane is done with it
            const int fc_in = N.fc_in, fc_out = N.fc_out;
            const float beta = N.beta;
            if (lane < fc_out) {
                const float *fw = s_fcw + lane * fc_in;
                float total = 0.0f;
                int d = 0;
                for (; d + 4 <= fc_in; d += 4) {                  // four weights in flight per round trip; the chain stays in order
                    const float w0 = fw[d], w1 = fw[d + 1], w2 = fw[d + 2], w3 = fw[d + 3];
                    const float x0 = vec[d], x1 = vec[d + 1], x2 = vec[d + 2], x3 = vec[d + 3];
                    const float p0 = x0 * w0, p1 = x1 * w1, p2 = x2 * w2, p3 = x3 * w3;
                    total += p0; total += p1; total += p2; total += p3;
                }
                for (; d < fc_in; ++d) {
                    const float prod = vec[d] * fw[d];
                    total += prod;
                }
                const float lgt = act_clamp(total + s_fcb[lane], N.fc_min, N.fc_max);
                lg[lane] = lgt;
                if (tap_logits) tap_logits[(size_t)clip * fc_out + lane] = lgt;
            }
            WAVE_SYNC();
            // softmax.h:31-63: max, then sum += exp((x - max) * beta) in class order, then exp(...) / sum.  Each lane evaluates
            // its own class's exponential once; the sum adds the same values in the same order
            float e_own = 0.0f;
            if (lane < fc_out) {
                float mx = -FLT_MAX;
                for (int c = 0; c < fc_out; ++c) mx = mx < lg[c] ? lg[c] : mx;
                e_own = expf((lg[lane] - mx) * beta);
                ex[lane] = e_own;
            }
            WAVE_SYNC();
            if (lane < fc_out) {
                float sum = 0.0f;
                for (int c = 0; c < fc_out; ++c) sum += ex[c];
                scores[(size_t)clip * fc_out + lane] = e_own / sum;
            }
            WAVE_SYNC();
        }
        mark(1 + KWS_MAX_BLOCKS);
    }
    if (profiling && lane == 0)
        for (int i = 0; i < KWS_MAX_BLOCKS + 2; ++i) prof[i] = ph[i];
}
