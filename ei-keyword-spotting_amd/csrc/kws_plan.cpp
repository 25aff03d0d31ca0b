// kws_plan.cpp -- execution plans.  Everything the reference recomputes per clip on the CPU but that does not depend on the
// audio is computed HERE once per model, with the reference's own formulas and precisions (each builder cites its source),
// and uploaded to HBM.
#include "kws_internal.h"
#include "kws_dct_tables.h"
#include <cstring>

template <int NF>
static bool dct_tables_match(const std::vector<float2> &tw, const std::vector<float2> &stw, const std::vector<float> &cs,
                             const std::vector<float> &sn, float s0, float s1)
{
    typedef KwsDctTab<NF> T;
    auto same = [](float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; };      // bit for bit (signed zeros too)
    if ((int)tw.size() != NF / 2 || (int)stw.size() != NF / 4 || (int)cs.size() != NF / 2 + 1 || (int)sn.size() != NF / 2 + 1) return false;
    for (int i = 0; i < NF / 2; ++i) if (!same(tw[i].x, T::tw_r[i]) || !same(tw[i].y, T::tw_i[i])) return false;
    for (int i = 0; i < NF / 4; ++i) if (!same(stw[i].x, T::stw_r[i]) || !same(stw[i].y, T::stw_i[i])) return false;
    for (int i = 0; i < NF / 2 + 1; ++i) if (!same(cs[i], T::cs[i]) || !same(sn[i], T::sn[i])) return false;
    return same(s0, T::s0) && same(s1, T::s1);
}

EI_IMPULSE_ERROR build_dsp_plan(kws_handle *h)
{
    const Model &m = h->model;
    const DspCfg &c = m.dsp;
    KwsDspPlan &P = h->dsp;
    const uint32_t fs = m.frequency;
    // framing: processing.hpp:194-284
    const int frame_len = (int)roundf((float)fs * c.frame_length);
    const float stride_f = roundf((float)fs * c.frame_stride);
    const int stride = (int)stride_f;
    if (frame_len < 1 || stride_f < 1.0f || (size_t)frame_len > (size_t)m.raw_sample_count || m.raw_sample_count > (1u << 30))
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "framing: %u samples, frame length %d, stride %g", m.raw_sample_count, frame_len, (double)stride_f);
    const size_t diff = (size_t)m.raw_sample_count - (size_t)frame_len;
    const int nfr = (int)floorf((float)diff / stride_f);
    P.n_samples = (int)m.raw_sample_count;
    P.n_frames = nfr;
    P.frame_stride = stride;
    P.frame_len = frame_len;
    P.fft_len = c.fft_length;
    P.n_bins = c.fft_length / 2 + 1;
    P.n_filters = c.num_filters;
    // columns of the feature matrix: cepstra, or -- MFE block (extract_mfe_features) -- the mel filters themselves
    const bool mfe = c.block == DSP_BLOCK_MFE;
    const int ncep = mfe ? c.num_filters : c.num_cepstral;
    P.n_cepstral = ncep;
    P.win_size = c.win_size;
    P.pad = (int)(uint16_t)((c.win_size - 1) / 2);
    P.pre_shift = c.pre_shift;
    P.pre_cof = mfe ? 0.0f : c.pre_cof;        // the MFE block hands the raw signal to feature::mfe (L432 ei_run_dsp.h:398-400)
    P.inv_fft = (float)(1.0 / (double)(float)c.fft_length);
    const int N = c.num_filters;
    P.dct_s0 = sqrtf(1.0f / (float)(4 * N));
    P.dct_s1 = sqrtf(1.0f / (float)(2 * N));

    // What the tuned kernel (kws_mfcc.hip) is instantiated for: fft 256, 32 or 40 filters, up to 52 frames, 16-byte aligned
    // frames, short mel filters.  Everything else the reference accepts goes to the general kernels (kws_generic.hip).
    if (c.axes != 1) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "MFCC block with %d axes", c.axes);
    const int used = std::min(frame_len, c.fft_length);
    if (c.fft_length < 4 || (c.fft_length & 1) || N < 2 || (N & 1) || N > 128 || c.pre_shift != 1 || (c.win_size & 1) == 0 || c.win_size < 1 ||
        nfr < 1 || stride < 1 || ncep < 1 || ncep > N || (long)(nfr - 1) * stride + used > (long)P.n_samples ||
        (size_t)nfr * ncep != m.nn_input_frame_size)
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "MFCC configuration outside the kernels (fft %d, filters %d, frames %d, frame_len %d, stride %d, "
                    "cepstra %d, win %d, shift %d)", c.fft_length, N, nfr, frame_len, stride, ncep, c.win_size, c.pre_shift);
    auto factor = [](int n, int *fac) {                         // kf_factor: 4s, then 2s, then 3, 5, 7 ...; returns levels or -1
        int p = 4, levels = 0;
        const double floor_sqrt = floor(sqrt((double)n));
        do {
            while (n % p) {
                switch (p) { case 4: p = 2; break; case 2: p = 3; break; default: p += 2; break; }
                if (p > floor_sqrt) p = n;
            }
            n /= p;
            if (p > 5 || levels >= 12) return -1;               // kf_bfly_generic (other primes) is not restated
            fac[2 * levels] = p; fac[2 * levels + 1] = n;
            levels++;
        } while (n > 1);
        return levels;
    };
    P.fft_levels = factor(c.fft_length / 2, P.fft_fac);
    P.dct_levels = factor(N / 2, P.dct_fac);
    if (P.fft_levels < 0 || P.dct_levels < 0)
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "fft_length %d / %d filters need a radix other than 2, 3, 4, 5", c.fft_length, N);
    const bool tuned = c.fft_length == 256 && (N == 32 || N == 40) && frame_len >= c.fft_length && nfr <= kws_mfcc_max_frames(N) &&
                       (stride * 2) % 16 == 0 && (P.n_samples * 2) % 16 == 0 && nfr + 2 * P.pad <= kws_mfcc_max_prow() &&
                       c.win_size <= kws_mfcc_max_win(ncep) && nfr <= kws_mfcc_max_frames_for(N, ncep) &&
                       c.win_size >= ((N == 40 && ncep > 16) ? 17 : 13) && nfr <= 4 * kws_mfcc_cmvn_rows();
    // the MFE block's tuned normalisation (kws_mfe_norm_kernel) walks cmvn_columns<17, 20> (more than 16 columns: 3 x 17 rows, a window of at least
    // 17 rows) or <13, 16> (4 x 13, 13); an MFE block outside it, or outside the tuned kernel altogether, is a general plan like any other:
    // the general spectral kernels write its mel rows and kws_mfe_norm_lds_kernel / the global-memory form normalise them (kws_generic.hip)
    const bool mfe_norm_tuned = nfr <= (N > 16 ? 51 : 52) && c.win_size >= (N > 16 ? 17 : 13);
    P.generic = (tuned && (!mfe || mfe_norm_tuned)) ? 0 : 1;
    // A general MFE plan is admitted from 32 filters up: the filter counts at which the restated block is pinned against the compiled reference
    // (32, 40, 64).  Below that an MFE block outside the tuned shape stays refused, as it always was.
    if (mfe && P.generic && N < 32)
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "MFE block: %d frames x %d filters, window %d: a general-shape MFE plan needs at least 32 filters", nfr, N,
                    c.win_size);
    // (MFE: frames have no predecessor sample, so any general MFE plan whose spectral stage fits the tuned kernel is chunkable)
    P.spectral_tuned = (P.generic && c.fft_length == 256 && (N == 32 || N == 40) && frame_len >= c.fft_length && (stride * 2) % 16 == 0 &&
                        (P.n_samples * 2) % 16 == 0) ? 1 : 0;
    P.wrap_index = P.n_samples - 1;

    std::vector<float2> tw, stw, dtw, dstw;
    h_twiddles(c.fft_length / 2, tw);
    h_super_twiddles(c.fft_length / 2, stw);
    h_twiddles(N / 2, dtw);
    h_super_twiddles(N / 2, dstw);
    std::vector<float> dcos(N / 2 + 1), dsin(N / 2 + 1);
    for (int i = 0; i < N / 2 + 1; i++) {                       // fast-dct-fft.cpp:71-74
        float temp = (float)((double)i * M_PI / (double)(N * 2));
        dcos[i] = cosf(temp);
        dsin[i] = sinf(temp);
    }
    // the kernel carries the DCT constants as literals (kws_dct_tables.h, tools/gen_dct_tables.cpp): they must be exactly
    // what this host computes in the reference's way, or the features would silently differ
    if (!P.generic) {
        bool same;
        if (N == 32) same = dct_tables_match<32>(dtw, dstw, dcos, dsin, P.dct_s0, P.dct_s1);
        else same = dct_tables_match<40>(dtw, dstw, dcos, dsin, P.dct_s0, P.dct_s1);
        if (!same) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "DCT constants of the kernel build differ from this host's (%d filters)", N);
    }
    const uint32_t high = c.high_frequency == 0 ? fs / 2 : (uint32_t)c.high_frequency;   // feature.hpp:203-205
    std::vector<float> fb = h_filterbank(N, P.n_bins, fs, (uint32_t)c.low_frequency, high, c.quantize_fb != 0);
    std::vector<int> fstart(N + 1, 0), fbin;
    std::vector<float> fw;
    int max_nz = 0;
    for (int j = 0; j < N; j++) {
        fstart[j] = (int)fbin.size();
        for (int k = 0; k < P.n_bins; k++) {
            const float w = fb[(size_t)k * N + j];
            if (w != 0.0f) { fbin.push_back(k); fw.push_back(w); }     // zero weights add an exact +0: skipped
        }
        max_nz = std::max(max_nz, (int)fbin.size() - fstart[j]);
    }
    fstart[N] = (int)fbin.size();
    P.max_nz = max_nz;
    P.filt_nnz = (int)fbin.size();
    if (max_nz > kws_mfcc_max_nz()) { P.generic = 1; P.spectral_tuned = 0; }      // the tuned kernel keeps a filter's taps in registers
    std::vector<int> pmap;
    h_pad_map(nfr, P.pad, pmap);

    EI_IMPULSE_ERROR e;
    if ((e = h->upload(tw, &P.tw))) return e;
    if ((e = h->upload(stw, &P.stw))) return e;
    if ((e = h->upload(dtw, &P.dct_tw))) return e;
    if ((e = h->upload(dstw, &P.dct_stw))) return e;
    if ((e = h->upload(dcos, &P.dct_cos))) return e;
    if ((e = h->upload(dsin, &P.dct_sin))) return e;
    if ((e = h->upload(fstart, &P.filt_start))) return e;
    if ((e = h->upload(fbin, &P.filt_bin))) return e;
    if ((e = h->upload(fw, &P.filt_w))) return e;
    if ((e = h->upload(pmap, &P.pad_map))) return e;
    return EI_IMPULSE_OK;
}

int kws_frames_for_length(const kws_handle *h, size_t n)
{
    const KwsDspPlan &P = h->dsp;
    const float stride_f = roundf((float)h->model.frequency * h->model.dsp.frame_stride);          // as build_dsp_plan
    if (n < (size_t)P.frame_len || n > (1u << 30)) return 0;
    return (int)floorf((float)(n - (size_t)P.frame_len) / stride_f);
}

EI_IMPULSE_ERROR kws_plan_for_length(kws_handle *h, size_t n, KwsDspPlan *out)
{
    const int nfr = kws_frames_for_length(h, n);
    if (nfr < 1 || nfr > h->dsp.n_frames) return fail(KWS_ERROR_BAD_ARGUMENT, "a window of %zu samples has %d frames (the model's: %d)", n, nfr, h->dsp.n_frames);
    *out = h->dsp;
    out->n_samples = (int)n;
    out->n_frames = nfr;
    if (nfr != h->dsp.n_frames) {
        auto it = h->pad_maps_by_rows.find(nfr);
        if (it == h->pad_maps_by_rows.end()) {
            std::vector<int> pmap;
            h_pad_map(nfr, out->pad, pmap);
            const int *d = nullptr;
            if (EI_IMPULSE_ERROR e = h->upload(pmap, &d)) return e;
            it = h->pad_maps_by_rows.emplace(nfr, d).first;
        }
        out->pad_map = it->second;
    }
    return EI_IMPULSE_OK;
}

static EI_IMPULSE_ERROR build_nn_plan_f32(kws_handle *h);

// (sum|w| * max(|-128 + in_off|, |127 + in_off|) + |bias|) << shift > 2^31 - 1: the largest |accumulator + bias| any int8 input
// can produce, shifted left as MultiplyByQuantizedMultiplier shifts it, leaves int32
static bool h_left_shift_overflows(int64_t wabs, int32_t in_off, int32_t bias, int shift)
{
    const int64_t xmax = std::max(std::llabs(-128ll + in_off), std::llabs(127ll + in_off));
    const int64_t bound = wabs * xmax + std::llabs((long long)bias);
    return shift > 30 || bound > (0x7fffffffll >> shift);
}

// SOFTMAX int8 -> int8 (softmax.cc:187-226): everything but the final reciprocal/rescale depends only on (max - x)
static EI_IMPULSE_ERROR build_softmax_tables(kws_handle *h, size_t i, int cur, const int32_t **sm_exp, const uint8_t **sm_valid)
{
    const Model &m = h->model;
    const Tensor &tout = m.t[m.t_out];
    if (i >= m.n.size() || m.n[i].op != OP_SOFTMAX || m.n[i].in[0] != cur || m.n[i].out[0] != (int)m.t_out || i + 1 != m.n.size())
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "expected a final SOFTMAX");
    const Node &sn = m.n[i];
    const Tensor &x = m.t[cur];
    if (tout.scale[0] != 1.f / 256 || tout.zero[0] != -128) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "softmax output quantisation");
    double rm = (double)sn.beta * (double)x.scale[0] * (double)(1 << (31 - 5));
    rm = std::min(rm, (double)((1ll << 31) - 1.0));
    int32_t mult; int left_shift;
    h_quantize_multiplier(rm, &mult, &left_shift);
    const double max_in = 1.0 * ((1 << 5) - 1) * (double)(1ll << (31 - 5)) / (double)(1ll << left_shift);
    const int diff_min = (int)(-1.0 * (double)(int)floor(max_in));
    std::vector<int32_t> ex(256);
    std::vector<uint8_t> valid(256);
    for (int d = 0; d < 256; d++) {
        const int32_t diff = -d;
        valid[d] = diff >= diff_min;
        const int32_t resc = h_srdhm((int32_t)((uint32_t)diff * (1u << left_shift)), mult);
        ex[d] = valid[d] ? h_exp_neg_q5_26(resc) : 0;
    }
    EI_IMPULSE_ERROR e;
    if ((e = h->upload(ex, sm_exp))) return e;
    if ((e = h->upload(valid, sm_valid))) return e;
    return EI_IMPULSE_OK;
}

static std::mutex g_handoff_mu;
static void handoff_init(kws_handle *h, size_t row_bytes)
{
    h->handoff.bytes = KWS_HANDOFF_BYTES;
    if (const char *ev = KWS_DEV_ENV("KWS_DEV_HANDOFF_BYTES")) { const long v = atol(ev); if (v > 0 && (size_t)v < KWS_HANDOFF_BYTES) h->handoff.bytes = (size_t)v; }
    if (h->handoff.bytes < row_bytes) h->handoff.bytes = row_bytes;          // at least one clip per chunk
}
void *kws_handoff_for(KwsHandoff *H, void *stream)
{
    std::lock_guard<std::mutex> lk(g_handoff_mu);
    for (auto &s_ : H->set) if (s_.used && s_.stream == stream) return s_.buf;
    for (auto &s_ : H->set)
        if (!s_.used) {
            if (hipMalloc(&s_.buf, H->bytes) != hipSuccess) { s_.buf = nullptr; return nullptr; }
            s_.used = 1; s_.stream = stream;
            return s_.buf;
        }
    // more streams than sets: a set changes hands once everything enqueued has finished with it
    if (hipDeviceSynchronize() != hipSuccess) return nullptr;
    auto &s_ = H->set[H->next];
    H->next = (H->next + 1) % KWS_HANDOFF_SETS;
    s_.stream = stream;
    return s_.buf;
}

// Is what starts at node i a dense stack?  A FULLY_CONNECTED that follows no conv block, or that is followed by another one.  Every graph
// served before keeps its kernels, and a single FULLY_CONNECTED behind conv blocks keeps the limits of those kernels' own head (KWS_FC_IN_MAX /
// KWS_FC_W_MAX): beyond them it is refused as it always was.
static bool h_dense_stack(const Model &m, size_t i, int n_blocks)
{
    if (i >= m.n.size() || m.n[i].op != OP_FULLY_CONNECTED) return false;
    if (n_blocks == 0) return true;
    size_t j = i + 1;
    while (j < m.n.size() && m.n[j].op == OP_RESHAPE) j++;
    return j < m.n.size() && m.n[j].op == OP_FULLY_CONNECTED;
}

// The dense stack of an int8 graph: 1 .. 4 FULLY_CONNECTED (fully_connected.cc:322-396, per-tensor quantisation) from node i on, whose
// first layer reads `inputs` values of the flowing tensor cur; then SOFTMAX.
static EI_IMPULSE_ERROR build_dense_i8(kws_handle *h, size_t i, int cur, int inputs)
{
    const Model &m = h->model;
    KwsNnPlan &N = h->nn;
    KwsDensePlan &D = h->dense;
    memset(&D, 0, sizeof(D));
    D.tap_off = h->pooled_tap_bytes;
    D.n_labels = N.n_labels;
    D.out_scale = N.out_scale; D.out_zp = N.out_zp;
    auto same_quant = [&](int a, int b) {
        return !m.t[a].scale.empty() && !m.t[b].scale.empty() && m.t[a].scale[0] == m.t[b].scale[0] && m.t[a].zero[0] == m.t[b].zero[0];
    };
    int k_in = inputs, lds_used = 0;
    D.act_stride = 64 + 16;
    while (i < m.n.size() && m.n[i].op == OP_FULLY_CONNECTED) {
        const int li = D.n_layers;
        if (li >= KWS_DENSE_MAX) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "more than %d FULLY_CONNECTED layers", KWS_DENSE_MAX);
        const Node &fc = m.n[i];
        if (fc.in[0] != cur) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "dense layer %d: input is not the flowing tensor", li);
        const Tensor &x = m.t[cur], &w = m.t[fc.in[1]], &y = m.t[fc.out[0]];
        const Tensor *bias = (fc.in.size() > 2 && fc.in[2] >= 0) ? &m.t[fc.in[2]] : nullptr;
        const long units = w.dims[0], k = w.dims[1];
        if (x.type != TYPE_I8 || w.type != TYPE_I8 || y.type != TYPE_I8 || x.scale.empty() || w.scale.empty() || y.scale.empty() || x.zero.empty() ||
            w.zero.empty() || y.zero.empty() || w.scale.size() != 1)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "dense layer %d: tensor types (int8, per-tensor quantisation)", li);
        if (k != k_in || k > KWS_DENSE_IN_MAX || units < 1 || units > KWS_DENSE_UNITS_MAX || units * k > KWS_DENSE_W_MAX || !w.is_const ||
            (long)w.nbytes != units * k || (long)w.data.size() < units * k || y.dims.back() != units || (long)y.nbytes != units)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "dense layer %d: weights [%ld][%ld] for %d inputs are outside the kernel's limits (%d units, %d inputs, %d bytes)",
                        li, units, k, k_in, KWS_DENSE_UNITS_MAX, KWS_DENSE_IN_MAX, KWS_DENSE_W_MAX);
        if (bias && (!bias->is_const || bias->type != TYPE_I32 || (long)bias->nbytes != units * 4 || (long)bias->data.size() < units * 4))
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "dense layer %d: bias", li);
        if (fc.p[0] < 0 || fc.p[0] > 3) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "dense layer %d: fused activation %d", li, fc.p[0]);
        KwsDenseLayer &L = D.l[li];
        L.k = (int)k; L.kpad = ((int)k + 63) & ~63; L.units = (int)units; L.upad = ((int)units + 15) & ~15;
        const int32_t in_off = -x.zero[0];
        L.w_off = -w.zero[0]; L.out_zp = y.zero[0];
        const double in_prod = (double)(x.scale[0] * w.scale[0]);     // kernel_util_lite.cc:160-172 (float product)
        int32_t mult; int exponent;
        h_quantize_multiplier(in_prod / (double)y.scale[0], &mult, &exponent);
        if (mult < 0 || exponent < -31) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "dense layer %d: requantisation multiplier", li);
        L.mult = mult; L.shift = exponent;
        int32_t amin, amax;
        h_act_range(fc.p[0], y.scale[0], y.zero[0], &amin, &amax);
        L.act_min = amin; L.act_max = amax;
        const int8_t *wd = (const int8_t *)w.data.data();
        const int32_t *bd = bias ? (const int32_t *)bias->data.data() : nullptr;
        std::vector<int32_t> beff((size_t)L.upad, 0);
        for (int o = 0; o < L.units; o++) {
            int64_t wsum = 0, wabs = 0;
            for (int d = 0; d < L.k; d++) { const int v = wd[(size_t)o * L.k + d]; wsum += v; wabs += std::abs(v + L.w_off); }
            const int32_t b = bd ? bd[o] : 0;
            // the same left-shift bound as the conv blocks
            if (exponent > 0 && h_left_shift_overflows(wabs, in_off, b, exponent))
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "dense layer %d unit %d: requantisation shifts left by %d and (sum|w| * max|x| + |bias|) << %d "
                            "can pass 2^31 - 1", li, o, exponent, exponent);
            beff[(size_t)o] = (int32_t)(uint32_t)((int64_t)b + (int64_t)in_off * wsum + (int64_t)L.k * in_off * L.w_off);
        }
        const int ks = L.kpad / 64;
        std::vector<int8_t> frag((size_t)L.upad * L.kpad, 0);
        for (int o = 0; o < L.units; o++)
            for (int d = 0; d < L.k; d++) {
                const int t = o >> 4, s_ = d >> 6, lane = (o & 15) + 16 * ((d & 63) >> 4);
                frag[(((size_t)t * ks + s_) * 64 + lane) * 16 + (d & 15)] = wd[(size_t)o * L.k + d];
            }
        L.lds_off = -1;
        if (lds_used + (int)frag.size() <= KWS_DENSE_LDS_W) { L.lds_off = lds_used; lds_used += (int)frag.size(); }
        EI_IMPULSE_ERROR e;
        if ((e = h->upload(frag, &L.wfrag))) return e;
        if ((e = h->upload(beff, &L.bias_eff))) return e;
        D.act_stride = std::max(D.act_stride, ((L.units + 63) & ~63) + 16);
        D.n_layers++;
        cur = fc.out[0];
        k_in = L.units;
        i++;
        while (i < m.n.size() && m.n[i].op == OP_RESHAPE && m.n[i].in[0] == cur) {
            if (!same_quant(cur, m.n[i].out[0])) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "reshape changes quantisation");
            cur = m.n[i].out[0];
            i++;
        }
    }
    if (D.n_layers == 0) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "expected FULLY_CONNECTED after the conv blocks");
    const KwsDenseLayer &last = D.l[D.n_layers - 1];
    if (last.units != N.n_labels || last.units > 48)
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "the last FULLY_CONNECTED has %d outputs for %d labels (at most 48)", last.units, N.n_labels);
    for (int li = 0; li + 1 < D.n_layers; li++) h->pooled_tap_bytes += D.l[li].units;
    D.lds_w_bytes = lds_used;
    if (EI_IMPULSE_ERROR e = build_softmax_tables(h, i, cur, &N.sm_exp, &N.sm_valid)) return e;
    D.sm_exp = N.sm_exp; D.sm_valid = N.sm_valid;
    N.fc_in = inputs; N.fc_out = 0;                      // the trunk form of kws_nn_kernel sizes its output vector by fc_in; it has no head
    N.dense = &D; N.handoff = &h->handoff;
    handoff_init(h, (size_t)inputs);
    h->n_dense = D.n_layers;
    if (N.n_blocks > 0 && kws_nn_smem_bytes(N, 4) > 158 * 1024)
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "int8 model needs %zu B of LDS in the generic network kernel (at most %d)", kws_nn_smem_bytes(N, 4), 158 * 1024);
    return EI_IMPULSE_OK;
}

// Stride and dilation of a conv node.  Both come from an untrusted blob, so they are bounded BEFORE any arithmetic on them: with
// 1 <= stride <= in_w <= KWS_NN_IMAGE_MAX, 1 <= taps <= 16 and (taps - 1) * dilation < KWS_NN_IMAGE_MAX every product and sum of h_out_size / h_pad_amount
// / nn_rows stays far inside an int.  Returns why the node is refused, or NULL.
#define KWS_NN_IMAGE_MAX 4096
static const char *h_conv_geometry_why(bool dw, int padding, int in_w, int f_w, int stride_w, int stride_h, int dil_w, int dil_h)
{
    if (stride_h != 1 || dil_h != 1) return "stride_h / dilation_height_factor other than 1 (only the time axis may be strided or dilated)";
    if (stride_w == 1 && dil_w == 1) return nullptr;
    if (in_w < 1 || in_w > KWS_NN_IMAGE_MAX || f_w < 1 || f_w > 16 || stride_w < 1 || stride_w > in_w || dil_w < 1 || dil_w >= KWS_NN_IMAGE_MAX ||
        (f_w - 1) * dil_w >= KWS_NN_IMAGE_MAX)
        return "stride / dilation outside the kernels' limits (1 <= stride <= input width, (taps - 1) * dilation below the 4096-row image bound)";
    if (dw && dil_w > 1 && padding != 2)
        return "SAME-padded depthwise with dilation > 1 is not served: the reference computes a depthwise convolution's padding with dilation 1 "
               "(depthwise_conv.cc:489-492) while its loops dilate, so its output is shifted";
    return nullptr;
}

// ---- 2-D convolutional graphs -------------------------------------------------------------------------------------------------------
// A graph belongs to the family when the tensor flowing into its first convolution is [1][H][W][C] with H > 1 and W > 1 (H: frames, W: cepstral / mel
// columns, as Keras' Reshape((frames, columns, 1)) lays them out).  [1][1][W][C] stays with the 1-D planner, its refusals included.
static bool h_is_2d(const Model &m, size_t i, int cur)
{
    if (i >= m.n.size() || (m.n[i].op != OP_CONV_2D && m.n[i].op != OP_DEPTHWISE_CONV_2D)) return false;
    const Tensor &x = m.t[cur];
    return x.dims.size() == 4 && x.dims[0] == 1 && x.dims[1] > 1 && x.dims[2] > 1;
}

// LDS of the 2-D trunks at n_waves waves per workgroup -- per workgroup the weights and per-channel constants of every block, per wave two ping-pong
// images, laid out as kws_nn2d_trunk_kernel / kws_nn2d_f32_trunk_kernel walk them -- and the wave count their launchers pick (kws_nn2d.h).  Host arithmetic
// on the plan alone, so it lives with the plan builder: kws_create refuses a graph that does not fit before any kernel is involved.
size_t kws_nn2d_smem_bytes(const KwsNn2dPlan &N, int n_waves)
{
    size_t s = 0;
    int img_b[2] = { 0, 0 };
    for (int b = 0; b < N.n_blocks; ++b) {
        const KwsConv2dBlock &k = N.blk[b];
        s += (((size_t)k.w_bytes + 15) & ~(size_t)15) + (size_t)k.g.out_c * 16;
        img_b[b & 1] = std::max(img_b[b & 1], kws_nn2d_img_bytes(k.g, 1));
    }
    return s + (size_t)n_waves * (size_t)(img_b[0] + img_b[1]);
}
int kws_nn2d_waves(const KwsNn2dPlan &N)
{
    for (int nw = KWS_NN2D_WAVES_MAX; nw >= KWS_NN2D_WAVES_MIN; --nw)
        if (kws_nn2d_smem_bytes(N, nw) <= KWS_NN2D_LDS_I8) return nw;
    return 0;
}
size_t kws_nn2d_f32_smem_bytes(const KwsNn2dPlanF32 &N, int n_waves)
{
    size_t s = 0;
    int img_b[2] = { 0, 0 };
    for (int b = 0; b < N.n_blocks; ++b) {
        const KwsConv2dGeom &g = N.blk[b].g;
        s += sizeof(float) * (size_t)(((g.out_c * g.kh * g.krow + 3) & ~3) + ((g.out_c + 3) & ~3));
        img_b[b & 1] = std::max(img_b[b & 1], kws_nn2d_img_bytes(g, 4));
    }
    return s + (size_t)n_waves * (size_t)(img_b[0] + img_b[1]);
}
int kws_nn2d_f32_waves(const KwsNn2dPlanF32 &N)
{
    for (int nw = KWS_NN2D_WAVES_MAX; nw >= KWS_NN2D_WAVES_MIN; --nw)
        if (kws_nn2d_f32_smem_bytes(N, nw) <= KWS_NN2D_LDS_F32) return nw;
    return 0;
}

struct H2dBlock { KwsConv2dGeom g; const Node *cv; int x_id, y_id, act, pool_act; };

// The blocks of a 2-D graph from conv node i on: CONV_2D [-> MAX_POOL_2D], RESHAPEs that keep the quantisation skipped.  Everything comes from an untrusted
// blob, so every dim, filter side and stride is bounded BEFORE any arithmetic on it (sides <= 1024, filters and pools <= 7, strides <= 7: every product of
// kernels/padding.h stays far inside an int).  On return i / cur stand behind the last block.
static EI_IMPULSE_ERROR h_nn2d_walk(const Model &m, size_t &i, int &cur, bool is_float, std::vector<H2dBlock> &blocks)
{
    const uint32_t want = is_float ? TYPE_F32 : TYPE_I8;
    auto same_quant = [&](int a, int b) {
        if (is_float) return true;
        return !m.t[a].scale.empty() && !m.t[b].scale.empty() && !m.t[a].zero.empty() && !m.t[b].zero.empty() && m.t[a].scale[0] == m.t[b].scale[0] &&
               m.t[a].zero[0] == m.t[b].zero[0];
    };
    auto skip_reshapes = [&]() {
        while (i < m.n.size() && m.n[i].op == OP_RESHAPE && m.n[i].in[0] == cur) {
            if (!same_quant(cur, m.n[i].out[0])) return false;
            cur = m.n[i].out[0];
            i++;
        }
        return true;
    };
    int ch = 0, cw = 0, cc = 0;
    while (i < m.n.size() && (m.n[i].op == OP_CONV_2D || m.n[i].op == OP_DEPTHWISE_CONV_2D)) {
        if ((int)blocks.size() >= KWS_MAX_BLOCKS) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "more than %d conv blocks", KWS_MAX_BLOCKS);
        const Node &cv = m.n[i];
        if (cv.op == OP_DEPTHWISE_CONV_2D)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu: DEPTHWISE_CONV_2D inside a 2-D graph is not served (the 2-D family is CONV_2D and MAX_POOL_2D)", i);
        if (cv.in[0] != cur) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu: input is not the flowing tensor", i);
        const Tensor &x = m.t[cur], &w = m.t[cv.in[1]], &y = m.t[cv.out[0]];
        const Tensor *bias = (cv.in.size() > 2 && cv.in[2] >= 0) ? &m.t[cv.in[2]] : nullptr;
        if (x.dims.size() != 4 || w.dims.size() != 4 || y.dims.size() != 4 || x.dims[0] != 1 || y.dims[0] != 1)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu: input, filter and output must be 4-D tensors of one batch", i);
        if (x.type != want || w.type != want || y.type != want) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu tensor types", i);
        H2dBlock B{};
        KwsConv2dGeom &g = B.g;
        g.in_h = x.dims[1]; g.in_w = x.dims[2]; g.in_c = x.dims[3];
        g.out_c = w.dims[0]; g.kh = w.dims[1]; g.kw = w.dims[2];
        if (g.in_h > KWS_NN2D_DIM_MAX || g.in_w > KWS_NN2D_DIM_MAX || g.in_c > 64 || g.out_c > 64 || g.kh > KWS_NN2D_K_MAX || g.kw > KWS_NN2D_K_MAX ||
            w.dims[3] != g.in_c)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu: a %d x %d filter over %d (filter: %d) -> %d channels on a %d x %d image is outside the 2-D kernels' "
                        "limits (filter sides 1 .. %d, at most 64 channels, image sides up to %d)", i, g.kh, g.kw, g.in_c, w.dims[3], g.out_c, g.in_h, g.in_w,
                        KWS_NN2D_K_MAX, KWS_NN2D_DIM_MAX);
        if (!w.is_const || (bias && (!bias->is_const || bias->type != (is_float ? TYPE_F32 : TYPE_I32) || (long)bias->nbytes != 4l * g.out_c)))
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu: the filter and the bias (%d values, %s) must be constants", i, g.out_c, is_float ? "float32" : "int32");
        const int padding = cv.p[0];
        g.sw = cv.p[1]; g.sh = cv.p[2]; B.act = cv.p[3];
        if (g.sh < 1 || g.sh > KWS_NN2D_STRIDE_MAX || g.sw < 1 || g.sw > KWS_NN2D_STRIDE_MAX)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu: stride %d x %d is outside 1 .. %d", i, g.sh, g.sw, KWS_NN2D_STRIDE_MAX);
        if (cv.p[4] != 1 || cv.p[5] != 1)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu: dilation %d x %d: a 2-D graph's convolutions are not dilated", i, cv.p[5], cv.p[4]);
        if ((padding != 1 && padding != 2) || B.act < 0 || B.act > 3)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu: padding %d / fused activation %d", i, padding, B.act);
        if (ch && (ch != g.in_h || cw != g.in_w || cc != g.in_c)) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "shape mismatch into conv %zu", i);
        g.out_h = h_out_size(padding, g.in_h, g.kh, g.sh, 1); g.out_w = h_out_size(padding, g.in_w, g.kw, g.sw, 1);
        if (g.out_h < 1 || g.out_w < 1 || y.dims[1] != g.out_h || y.dims[2] != g.out_w || y.dims[3] != g.out_c)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu output shape: the tensor is %d x %d x %d, kernels/padding.h gives %d x %d x %d", i, y.dims[1], y.dims[2],
                        y.dims[3], g.out_h, g.out_w, g.out_c);
        g.pad_t = h_pad_amount(g.sh, 1, g.in_h, g.kh, g.out_h); g.pad_l = h_pad_amount(g.sw, 1, g.in_w, g.kw, g.out_w);
        B.cv = &cv; B.x_id = cur; B.y_id = cv.out[0];
        cur = cv.out[0];
        i++;
        if (!skip_reshapes()) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "reshape changes quantisation");
        if (i < m.n.size() && m.n[i].op == OP_ADD)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "ADD %zu: a per-channel ADD inside a 2-D graph is not served (its convolutions carry their bias and activation)", i);
        g.ph = g.pw = g.psh = g.psw = 1; g.ppt = g.ppl = 0; g.has_pool = 0;
        g.pool_h = g.out_h; g.pool_w = g.out_w;
        if (i < m.n.size() && m.n[i].op == OP_MAX_POOL_2D) {
            const Node &pl = m.n[i];
            if (pl.in[0] != cur || !same_quant(cur, pl.out[0])) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool %zu input", i);
            const Tensor &px = m.t[cur], &py = m.t[pl.out[0]];
            if (px.dims.size() != 4 || py.dims.size() != 4 || px.dims[1] != g.out_h || px.dims[2] != g.out_w || px.dims[3] != g.out_c || py.type != want)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool %zu: its input is not the convolution's %d x %d x %d output", i, g.out_h, g.out_w, g.out_c);
            g.psw = pl.p[1]; g.psh = pl.p[2]; g.pw = pl.p[3]; g.ph = pl.p[4]; B.pool_act = pl.p[5];
            if (g.ph < 1 || g.ph > KWS_NN2D_K_MAX || g.pw < 1 || g.pw > KWS_NN2D_K_MAX || g.psh < 1 || g.psh > KWS_NN2D_K_MAX || g.psw < 1 || g.psw > KWS_NN2D_K_MAX)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool %zu: window %d x %d / stride %d x %d is outside 1 .. %d", i, g.ph, g.pw, g.psh, g.psw, KWS_NN2D_K_MAX);
            if ((pl.p[0] != 1 && pl.p[0] != 2) || B.pool_act < 0 || B.pool_act > 3 || (!is_float && B.pool_act != 0))
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool %zu: padding %d / fused activation %d", i, pl.p[0], B.pool_act);
            g.pool_h = h_out_size(pl.p[0], g.out_h, g.ph, g.psh, 1); g.pool_w = h_out_size(pl.p[0], g.out_w, g.pw, g.psw, 1);
            if (g.pool_h < 1 || g.pool_w < 1 || py.dims[0] != 1 || py.dims[1] != g.pool_h || py.dims[2] != g.pool_w || py.dims[3] != g.out_c)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool %zu output shape: the tensor is %d x %d x %d, kernels/padding.h gives %d x %d x %d", i, py.dims[1],
                            py.dims[2], py.dims[3], g.pool_h, g.pool_w, g.out_c);
            g.ppt = h_pad_amount(g.psh, 1, g.out_h, g.ph, g.pool_h); g.ppl = h_pad_amount(g.psw, 1, g.out_w, g.pw, g.pool_w);
            // every window holds a value of the image (SAME: the last window may be ragged; a stride past the window skips values, never leaves the image)
            if ((g.pool_h - 1) * g.psh - g.ppt >= g.out_h || (g.pool_w - 1) * g.psw - g.ppl >= g.out_w || g.ppt >= g.ph || g.ppl >= g.pw)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool %zu: a window lies outside the image", i);
            g.has_pool = 1;
            cur = pl.out[0];
            i++;
            if (!skip_reshapes()) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "reshape changes quantisation");
        }
        // the padded image: what the furthest tap of the last output reads, and at least the image behind its padding (VALID: trailing rows / columns no
        // output reads are staged all the same)
        g.img_rows = std::max(g.pad_t + g.in_h, (g.out_h - 1) * g.sh + g.kh);
        g.img_cols = std::max(g.pad_l + g.in_w, (g.out_w - 1) * g.sw + g.kw);
        g.krow = g.kw * g.in_c; g.krow4 = (g.krow + 3) & ~3;
        const int row = g.img_cols * g.in_c;
        g.img_pitch = is_float ? (row | 1) : 4 * (((row + 3) / 4) | 1);             // an odd number of dwords
        ch = g.pool_h; cw = g.pool_w; cc = g.out_c;
        blocks.push_back(B);
    }
    return EI_IMPULSE_OK;
}

static EI_IMPULSE_ERROR build_nn2d_i8(kws_handle *h, size_t &i, int &cur)
{
    const Model &m = h->model;
    KwsNn2dPlan &P = h->nn2d;
    memset(&P, 0, sizeof(P));
    std::vector<H2dBlock> blocks;
    if (EI_IMPULSE_ERROR e = h_nn2d_walk(m, i, cur, false, blocks)) return e;
    P.n_features = (int)m.nn_input_frame_size;
    if (blocks[0].g.in_h * blocks[0].g.in_w * blocks[0].g.in_c != P.n_features)
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "first conv does not consume the feature vector");
    for (size_t b = 0; b < blocks.size(); b++) {
        const H2dBlock &B = blocks[b];
        const Node &cv = *B.cv;
        const Tensor &x = m.t[B.x_id], &w = m.t[cv.in[1]], &y = m.t[B.y_id];
        const Tensor *bias = (cv.in.size() > 2 && cv.in[2] >= 0) ? &m.t[cv.in[2]] : nullptr;
        KwsConv2dBlock &k = P.blk[b];
        k.g = B.g;
        const KwsConv2dGeom &g = k.g;
        k.in_zp = x.zero[0]; k.out_zp = y.zero[0];
        h_act_range(B.act, y.scale[0], y.zero[0], &k.act_min, &k.act_max);
        // weights -> [out_c][kh][krow4]: a filter row's kw * in_c operands are contiguous in the NHWC image too; zero padded to whole dot4 words
        // bias_eff = bias + input_offset * sum(w)   (integer_ops/conv.h:64-113)
        std::vector<int8_t> wp((size_t)g.out_c * g.kh * g.krow4, 0);
        k.w_bytes = (int)wp.size();
        std::vector<int32_t> beff(g.out_c), mult(g.out_c), shift(g.out_c);
        const int8_t *wd = (const int8_t *)w.data.data();
        const int32_t *bd = bias ? (const int32_t *)bias->data.data() : nullptr;
        const int32_t in_off = -x.zero[0];
        const bool per_channel = w.scale.size() > 1;
        if (w.data.size() < (size_t)g.out_c * g.kh * g.krow || (bias && bias->data.size() < (size_t)g.out_c * 4))
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv block %zu: constant data", b);
        if (per_channel && ((int)w.scale.size() != g.out_c || w.qdim != 0)) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv block %zu: per-channel scale count", b);
        for (int oc = 0; oc < g.out_c; oc++) {
            int64_t wsum = 0, wabs = 0;
            for (int fy = 0; fy < g.kh; fy++)
                for (int j = 0; j < g.krow; j++) {
                    const int8_t v = wd[((size_t)oc * g.kh + fy) * g.krow + j];
                    wp[((size_t)oc * g.kh + fy) * g.krow4 + j] = v;
                    wsum += v; wabs += std::abs((int)v);
                }
            beff[oc] = (int32_t)((bd ? bd[oc] : 0) + (int64_t)in_off * wsum);
            const double eff = (double)x.scale[0] * (double)(per_channel ? w.scale[oc] : w.scale[0]) / (double)y.scale[0];
            int sh;
            h_quantize_multiplier(eff, &mult[oc], &sh);          // kernel_util_lite.cc:89-103
            shift[oc] = sh;
            if (mult[oc] < 0 || sh < -31) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv block %zu channel %d: requantisation multiplier", b, oc);
            // the left-shift bound of DESIGN 4.2, as for the 1-D blocks: the kernel pools raw accumulators on the strength of a monotonic requantisation
            if (sh > 0 && h_left_shift_overflows(wabs, in_off, bd ? bd[oc] : 0, sh))
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv block %zu channel %d: requantisation shifts left by %d and (sum|w| * max|x| + |bias|) << %d "
                            "can pass 2^31 - 1", b, oc, sh, sh);
        }
        EI_IMPULSE_ERROR e;
        if ((e = h->upload(wp, &k.w))) return e;
        if ((e = h->upload(beff, &k.bias_eff))) return e;
        if ((e = h->upload(mult, &k.mult))) return e;
        if ((e = h->upload(shift, &k.shift))) return e;
        P.tap_bytes += g.pool_h * g.pool_w * g.out_c;
        P.n_blocks++;
    }
    const KwsConv2dGeom &lg = P.blk[P.n_blocks - 1].g;
    P.out_n = lg.pool_h * lg.pool_w * lg.out_c;
    if (kws_nn2d_waves(P) == 0)
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "int8 2-D model needs %zu B of LDS at %d waves per workgroup (at most %d): its images do not fit the kernel's LDS budget",
                    kws_nn2d_smem_bytes(P, KWS_NN2D_WAVES_MIN), KWS_NN2D_WAVES_MIN, 158 * 1024);
    h->pooled_tap_bytes += P.tap_bytes;
    h->n_conv2d = P.n_blocks;
    return EI_IMPULSE_OK;
}

// residual graphs (below, behind the float helpers)
static bool h_is_residual(const Model &m);
static bool h_is_dw2d(const Model &m);
static EI_IMPULSE_ERROR build_nnres_i8(kws_handle *h, size_t &i, int &cur);

// Recognise the Edge Impulse 1-D CNN family and fold its per-model constants.
EI_IMPULSE_ERROR build_nn_plan(kws_handle *h)
{
    const Model &m = h->model;
    KwsNnPlan &N = h->nn;
    memset(&N, 0, sizeof(N));
    const Tensor &tin = m.t[m.t_in], &tout = m.t[m.t_out];
    if (tin.type == TYPE_F32 && tout.type == TYPE_F32) return build_nn_plan_f32(h);
    if (tin.type != TYPE_I8 || tout.type != TYPE_I8 || tin.scale.empty() || tout.scale.empty())
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "only int8-quantised and float32 models are implemented");
    N.n_features = (int)m.nn_input_frame_size;
    N.in_scale = tin.scale[0]; N.in_zp = tin.zero[0];
    N.out_scale = tout.scale[0]; N.out_zp = tout.zero[0];
    N.n_labels = (int)m.labels.size();

    int cur = (int)m.t_in;       // tensor currently flowing through the graph
    int cur_w = 0, cur_c = 0;    // logical [time][channel] shape once known
    size_t i = 0;
    auto same_quant = [&](int a, int b) {
        return !m.t[a].scale.empty() && !m.t[b].scale.empty() && m.t[a].scale[0] == m.t[b].scale[0] && m.t[a].zero[0] == m.t[b].zero[0];
    };
    auto skip_reshapes = [&]() {
        while (i < m.n.size() && m.n[i].op == OP_RESHAPE && m.n[i].in[0] == cur) {
            if (!same_quant(cur, m.n[i].out[0])) return false;
            cur = m.n[i].out[0];
            i++;
        }
        return true;
    };
    if (h_is_residual(m) || h_is_dw2d(m)) {
        // a residual graph or a 2-D graph with depthwise steps: its steps in a plan of their own, then the dense stack -- always,
        // as for a 2-D graph
        if (EI_IMPULSE_ERROR e = build_nnres_i8(h, i, cur)) return e;
        if (EI_IMPULSE_ERROR e = build_dense_i8(h, i, cur, h->nnres.out_n)) return e;
        h->handoff.trunkres = &h->nnres;
        return EI_IMPULSE_OK;
    }
    if (!skip_reshapes()) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "reshape changes quantisation");
    if (h_is_2d(m, i, cur)) {
        // a 2-D graph: its blocks in a plan of their own, then the dense stack -- always, a single FULLY_CONNECTED included
        if (EI_IMPULSE_ERROR e = build_nn2d_i8(h, i, cur)) return e;
        if (i >= m.n.size() || m.n[i].op != OP_FULLY_CONNECTED) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "expected FULLY_CONNECTED after the conv blocks");
        if (EI_IMPULSE_ERROR e = build_dense_i8(h, i, cur, h->nn2d.out_n)) return e;
        h->handoff.trunk2d = &h->nn2d;
        return EI_IMPULSE_OK;
    }
    while (i < m.n.size() && (m.n[i].op == OP_CONV_2D || m.n[i].op == OP_DEPTHWISE_CONV_2D)) {
        if (N.n_blocks >= KWS_MAX_BLOCKS) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "more than %d conv blocks", KWS_MAX_BLOCKS);
        const Node &cv = m.n[i];
        const bool dw = cv.op == OP_DEPTHWISE_CONV_2D;
        if (cv.in[0] != cur || cv.in.size() < 2) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv input is not the flowing tensor");
        const Tensor &x = m.t[cur], &w = m.t[cv.in[1]], &y = m.t[cv.out[0]];
        const Tensor *bias = (cv.in.size() > 2 && cv.in[2] >= 0) ? &m.t[cv.in[2]] : nullptr;
        const int in_h = x.dim4(1), in_w = x.dim4(2), in_c = x.dim4(3);
        const int out_c = dw ? w.dim4(3) : w.dim4(0), f_h = w.dim4(1), f_w = w.dim4(2);
        const int depth_mult = dw ? cv.p[6] : 1;
        const int padding = cv.p[0], stride_w = cv.p[1], stride_h = cv.p[2], act = cv.p[3], dil_w = cv.p[4], dil_h = cv.p[5];
        if (x.dim4(0) != 1 || in_h != 1 || f_h != 1 || !w.is_const ||
            (dw ? (w.dim4(0) != 1 || depth_mult < 1 || out_c != in_c * depth_mult) : (w.dim4(3) != in_c)) || (bias && !bias->is_const) ||
            f_w > 16 || out_c > 64 || x.dims.size() != 4 || (size_t)w.nbytes != (size_t)out_c * f_w * (dw ? 1 : in_c))
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu is not a 1xK (depthwise) convolution over time", i);
        if (const char *why = h_conv_geometry_why(dw, padding, in_w, f_w, stride_w, stride_h, dil_w, dil_h))
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu: %s (stride %d x %d, dilation %d x %d)", i, why, stride_w, stride_h, dil_w, dil_h);
        if (cur_w && (cur_w != in_w || cur_c != in_c)) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "shape mismatch into conv %zu", i);
        if (bias && (bias->type != TYPE_I32 || (int)bias->nbytes != out_c * 4)) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu bias", i);
        if (w.type != TYPE_I8 || x.type != TYPE_I8 || y.type != TYPE_I8) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu tensor types", i);
        const int out_w = h_out_size(padding, in_w, f_w, stride_w, dil_w);         // padding.h with the real stride and dilation; a negative total padding is 0
        const int pad_left = h_pad_amount(stride_w, dil_w, in_w, f_w, out_w);
        if (out_w < 1 || out_w != y.dim4(2) || y.dim4(3) != out_c)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu output shape: the tensor has %d rows, stride %d and dilation %d give %d", i, y.dim4(2), stride_w, dil_w, out_w);
        KwsConvBlock &k = N.blk[N.n_blocks];
        k.in_w = in_w; k.in_c = in_c; k.in_cpad = (in_c + 15) & ~15; k.out_c = out_c; k.taps = f_w; k.pad_left = pad_left;
        k.out_w = out_w; k.in_zp = x.zero[0]; k.out_zp = y.zero[0];
        k.stride = (short)stride_w; k.dilation = (short)dil_w;         // (both below KWS_NN_IMAGE_MAX: h_conv_geometry_why)
        k.depthwise = dw ? 1 : 0; k.depth_mult = depth_mult;
        h_act_range(act, y.scale[0], y.zero[0], &k.act_min, &k.act_max);
        // the reference's int8 depthwise op clamps to the int8 range whatever its fused activation says
        // (TFL/micro/kernels/depthwise_conv.cc:618-620, "TODO(b/130439627)") -- pinned in tests/test_oracle_vs_reference.py
        if (dw) { k.act_min = -128; k.act_max = 127; }
        // weights -> [out_c][taps][in_cpad] (depthwise: [out_c][taps padded to 4], from the filter's [taps][out_c]);
        // bias_eff = bias + input_offset * sum(w)   (integer_ops/conv.h:64-113, depthwise_conv.h:64-106)
        const int tp4 = (f_w + 3) & ~3;
        std::vector<int8_t> wp(dw ? (size_t)out_c * tp4 : (size_t)out_c * f_w * k.in_cpad, 0);
        k.w_bytes = (int)wp.size();
        std::vector<int32_t> beff(out_c), mult(out_c), shift(out_c);
        const int8_t *wd = (const int8_t *)w.data.data();
        const int32_t in_off = -x.zero[0];
        const bool per_channel = w.scale.size() > 1;
        if (per_channel && (int)w.scale.size() != out_c) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "per-channel scale count");
        for (int oc = 0; oc < out_c; oc++) {
            int64_t wsum = 0, wabs = 0;
            for (int tap = 0; tap < f_w; tap++) {
                if (dw) {
                    const int8_t v = wd[(size_t)tap * out_c + oc];
                    wp[(size_t)oc * tp4 + tap] = v;
                    wsum += v; wabs += std::abs((int)v);
                    continue;
                }
                for (int c = 0; c < in_c; c++) {
                    const int8_t v = wd[((size_t)oc * f_w + tap) * in_c + c];
                    wp[((size_t)oc * f_w + tap) * k.in_cpad + c] = v;
                    wsum += v; wabs += std::abs((int)v);
                }
            }
            beff[oc] = (int32_t)((bias ? ((const int32_t *)bias->data.data())[oc] : 0) + (int64_t)in_off * wsum);
            const double eff = (double)x.scale[0] * (double)(per_channel ? w.scale[oc] : w.scale[0]) / (double)y.scale[0];
            int sh;
            h_quantize_multiplier(eff, &mult[oc], &sh);          // kernel_util_lite.cc:89-103
            shift[oc] = sh;
            if (mult[oc] < 0) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "negative requantisation multiplier");
            // A multiplier of 1 or more shifts the accumulator LEFT before the multiplication (common.h:138-162).  Past 2^31 that is a
            // signed overflow in the reference (undefined), and a wrap here: requantisation then stops being monotonic, and the kernels
            // pool raw accumulators on the strength of that (kws_nn_int8_dev.h).  Refused when any input could reach the overflow.
            if (sh > 0 && h_left_shift_overflows(wabs, in_off, bias ? ((const int32_t *)bias->data.data())[oc] : 0, sh))
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv block %d channel %d: requantisation shifts left by %d and (sum|w| * max|x| + |bias|) << %d "
                            "can pass 2^31 - 1", N.n_blocks, oc, sh, sh);
        }
        cur = cv.out[0]; cur_w = out_w; cur_c = out_c;
        i++;
        if (!skip_reshapes()) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "reshape changes quantisation");
        // optional ADD(const per-channel tensor) with fused activation -> 256-entry table per channel
        std::vector<int8_t> lut((size_t)out_c * 256);
        for (int c = 0; c < out_c; c++) for (int v = 0; v < 256; v++) lut[(size_t)c * 256 + v] = (int8_t)(v - 128);
        k.has_lut = 0;
        if (i < m.n.size() && m.n[i].op == OP_ADD) {
            k.has_lut = 1;
            const Node &ad = m.n[i];
            int a_id = ad.in[0], b_id = ad.in[1];
            if (a_id != cur && b_id == cur) std::swap(a_id, b_id);
            const Tensor &t1 = m.t[ad.in[0]], &t2 = m.t[ad.in[1]], &to = m.t[ad.out[0]];
            const Tensor &cb = m.t[b_id];
            if (a_id != cur || !cb.is_const || cb.type != TYPE_I8 || (int)cb.nbytes != out_c || cb.dims.back() != out_c ||
                t1.type != TYPE_I8 || t2.type != TYPE_I8 || to.type != TYPE_I8)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "ADD %zu is not a per-channel constant int8 add", i);
            // CalculateOpData, add.cc:271-309
            const int left_shift = 20;
            const double twice_max = 2 * (double)std::max(t1.scale[0], t2.scale[0]);
            int32_t m1, m2, mo; int s1, s2, so;
            h_quantize_multiplier((double)t1.scale[0] / twice_max, &m1, &s1);
            h_quantize_multiplier((double)t2.scale[0] / twice_max, &m2, &s2);
            h_quantize_multiplier(twice_max / ((double)(1 << left_shift) * (double)to.scale[0]), &mo, &so);
            int32_t amin, amax;
            h_act_range(ad.p[0], to.scale[0], to.zero[0], &amin, &amax);
            const bool cur_is_first = (ad.in[0] == cur);
            for (int c = 0; c < out_c; c++) {
                const int8_t cval = ((const int8_t *)cb.data.data())[c];
                int prev = -129;
                for (int v = -128; v <= 127; v++) {
                    const int32_t x1 = cur_is_first ? v : cval, x2 = cur_is_first ? cval : v;
                    const int32_t v1 = -t1.zero[0] + x1, v2 = -t2.zero[0] + x2;           // integer_ops/add.h:108-131
                    const int32_t q1 = h_rdivpot(h_srdhm(v1 * (1 << left_shift), m1), -s1);
                    const int32_t q2 = h_rdivpot(h_srdhm(v2 * (1 << left_shift), m2), -s2);
                    int32_t o = h_rdivpot(h_srdhm(q1 + q2, mo), -so) + to.zero[0];
                    o = std::min(amax, std::max(amin, o));
                    if (o < prev) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "ADD table not monotonic");
                    prev = o;
                    lut[(size_t)c * 256 + (v + 128)] = (int8_t)o;
                }
            }
            cur = ad.out[0];
            i++;
            if (!skip_reshapes()) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "reshape changes quantisation");
        }
        // MAX_POOL_2D over time (optional: pool 1 = identity)
        k.pool = 1; k.pool_stride = 1; k.pool_w = out_w;
        if (i < m.n.size() && m.n[i].op == OP_MAX_POOL_2D) {
            const Node &pl = m.n[i];
            const Tensor &px = m.t[pl.in[0]], &py = m.t[pl.out[0]];
            if (pl.in[0] != cur || !same_quant(cur, pl.out[0])) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool %zu input", i);
            const int ph = px.dim4(1), pw = px.dim4(2);
            int f, s, out_n;
            if (pw == 1 && ph == cur_w) { f = pl.p[4]; s = pl.p[2]; if (pl.p[3] != 1) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "2-D pool"); out_n = py.dim4(1); }
            else if (ph == 1 && pw == cur_w) { f = pl.p[3]; s = pl.p[1]; if (pl.p[4] != 1) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "2-D pool"); out_n = py.dim4(2); }
            else return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool %zu is not over the time axis", i);
            const int po = h_out_size(pl.p[0], cur_w, f, s, 1);
            if (po != out_n || h_pad_amount(s, 1, cur_w, f, po) != 0 || (po - 1) * s >= cur_w || f > 8 || pl.p[5] != 0)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool %zu window/padding outside the kernel's limits", i);
            k.pool = f; k.pool_stride = s; k.pool_w = po;
            cur = pl.out[0]; cur_w = po;
            i++;
            if (!skip_reshapes()) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "reshape changes quantisation");
        }
        // un-pooled CONV_2D blocks (e.g. the pointwise halves of a depthwise-separable CNN) run on the matrix cores in the
        // generic kernel: 16-byte k-groups need activation rows of 16, 32 or 64 bytes
        k.mfma = (!dw && k.pool == 1 && in_c <= 64 && out_c <= 32 && out_w <= 64 && f_w <= 8 && stride_w == 1 && dil_w == 1) ? 1 : 0;      // (its tiles read contiguous rows)
        if (k.mfma) {
            const int cp = in_c <= 16 ? 16 : in_c <= 32 ? 32 : 64;
            if (cp != k.in_cpad) {
                std::vector<int8_t> w2((size_t)out_c * f_w * cp, 0);
                for (int r = 0; r < out_c * f_w; r++) std::memcpy(&w2[(size_t)r * cp], &wp[(size_t)r * k.in_cpad], (size_t)in_c);
                wp.swap(w2);
                k.in_cpad = cp;
                k.w_bytes = (int)wp.size();
            }
        }
        EI_IMPULSE_ERROR e;
        if ((e = h->upload(wp, &k.w))) return e;
        if ((e = h->upload(beff, &k.bias_eff))) return e;
        if ((e = h->upload(mult, &k.mult))) return e;
        if ((e = h->upload(shift, &k.shift))) return e;
        if ((e = h->upload(lut, &k.add_lut))) return e;
        h->pooled_tap_bytes += k.pool_w * k.out_c;
        N.n_blocks++;
    }
    if (N.n_blocks > 0 && N.blk[0].in_w * N.blk[0].in_c != N.n_features) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "first conv does not consume the feature vector");
    for (int b = 0; b + 1 < N.n_blocks; b++)
        if (N.blk[b].pool_w != N.blk[b + 1].in_w || N.blk[b].out_c != N.blk[b + 1].in_c)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv blocks do not chain");
    // no block, or more than one FULLY_CONNECTED: a dense stack
    if (h_dense_stack(m, i, N.n_blocks))
        return build_dense_i8(h, i, cur, N.n_blocks ? N.blk[N.n_blocks - 1].pool_w * N.blk[N.n_blocks - 1].out_c : N.n_features);
    if (N.n_blocks == 0) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "graph does not start with a convolution block");
    // FULLY_CONNECTED (fully_connected.cc:322-396)
    if (i < m.n.size() && m.n[i].op == OP_FULLY_CONNECTED && (m.t[m.n[i].in[1]].type != TYPE_I8 || m.t[m.n[i].out[0]].type != TYPE_I8))
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "FULLY_CONNECTED tensor types");
    if (i >= m.n.size() || m.n[i].op != OP_FULLY_CONNECTED || m.n[i].in[0] != cur)
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "expected FULLY_CONNECTED after the conv blocks");
    {
        const Node &fc = m.n[i];
        const Tensor &x = m.t[cur], &w = m.t[fc.in[1]], &y = m.t[fc.out[0]];
        const Tensor *bias = (fc.in.size() > 2 && fc.in[2] >= 0) ? &m.t[fc.in[2]] : nullptr;
        N.fc_in = w.dims.back(); N.fc_out = w.dims[0];
        const KwsConvBlock &lb = N.blk[N.n_blocks - 1];
        if (N.fc_in != lb.pool_w * lb.out_c || N.fc_in > KWS_FC_IN_MAX || N.fc_in * N.fc_out > KWS_FC_W_MAX || N.fc_out > 48 || N.fc_out != N.n_labels || !w.is_const ||
            w.type != TYPE_I8 || (int)w.nbytes != N.fc_in * N.fc_out || y.type != TYPE_I8 ||
            (bias && (!bias->is_const || bias->type != TYPE_I32 || (int)bias->nbytes != N.fc_out * 4)))
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "FULLY_CONNECTED shape %dx%d outside the kernel's limits", N.fc_out, N.fc_in);
        N.fc_in_off = -x.zero[0]; N.fc_w_off = -w.zero[0]; N.fc_out_zp = y.zero[0];
        const double in_prod = (double)(x.scale[0] * w.scale[0]);     // kernel_util_lite.cc:160-172 (float product)
        int32_t mult; int exponent;
        h_quantize_multiplier(in_prod / (double)y.scale[0], &mult, &exponent);
        N.fc_mult = mult; N.fc_shift = exponent;
        h_act_range(fc.p[0], y.scale[0], y.zero[0], &N.fc_act_min, &N.fc_act_max);
        for (int o = 0; exponent > 0 && o < N.fc_out; o++) {                      // the same left-shift bound as the conv blocks
            int64_t wabs = 0;
            for (int d = 0; d < N.fc_in; d++) wabs += std::abs((int)((const int8_t *)w.data.data())[(size_t)o * N.fc_in + d] + N.fc_w_off);
            if (h_left_shift_overflows(wabs, N.fc_in_off, bias ? ((const int32_t *)bias->data.data())[o] : 0, exponent))
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "FULLY_CONNECTED output %d: requantisation shifts left by %d and (sum|w| * max|x| + |bias|) << %d "
                            "can pass 2^31 - 1", o, exponent, exponent);
        }
        std::vector<int8_t> wv((const int8_t *)w.data.data(), (const int8_t *)w.data.data() + w.nbytes);
        std::vector<int32_t> bv(N.fc_out, 0);
        if (bias) memcpy(bv.data(), bias->data.data(), sizeof(int32_t) * N.fc_out);
        EI_IMPULSE_ERROR e;
        if ((e = h->upload(wv, &N.fc_w))) return e;
        if ((e = h->upload(bv, &N.fc_bias))) return e;
        cur = fc.out[0];
        i++;
    }
    if (EI_IMPULSE_ERROR e = build_softmax_tables(h, i, cur, &N.sm_exp, &N.sm_valid)) return e;
    // the generic kernel keeps every block's weights and ADD tables in LDS: a model that does not fit fails here, at load time,
    // not at its first inference
    if (!kws_nn_uses_mfma(N) && kws_nn_smem_bytes(N, 4) > 158 * 1024)
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "int8 model needs %zu B of LDS in the generic network kernel (at most %d)",
                    kws_nn_smem_bytes(N, 4), 158 * 1024);
    return EI_IMPULSE_OK;
}

// The same graph family with float32 tensors (the "fp32" configuration of BASELINE.json): constants are uploaded as they
// are, the fused activations become clamp ranges (kernel_util_lite.h:79-97 CalculateActivationRange<float>).
static void h_act_range_f32(int act, float *lo, float *hi)
{
    *lo = -FLT_MAX; *hi = FLT_MAX;                       // kTfLiteActNone: numeric_limits lowest()/max()
    if (act == 1) { *lo = 0.f; }                         // kTfLiteActRelu
    else if (act == 2) { *lo = -1.f; *hi = 1.f; }        // kTfLiteActReluN1To1
    else if (act == 3) { *lo = 0.f; *hi = 6.f; }         // kTfLiteActRelu6
}

// A multiplied constant (conv / depthwise / FULLY_CONNECTED weight) must be finite.  The kernels' zero-padded image rows multiply every weight of an
// out-of-image tap by 0 where the reference skips the tap (conv.h:71-75, depthwiseconv_float.h:71-75): 0 * w is an exact 0 only for a finite w
// (0 * inf = NaN).  FULLY_CONNECTED weights are held to the same condition so that one rule covers every multiplied constant.  Biases and ADD
// constants are added, never multiplied by padding: no condition.  Returns the index of the first non-finite value, or -1.
static long h_first_non_finite(const std::vector<float> &v)
{
    for (size_t i = 0; i < v.size(); ++i)
        if (!std::isfinite(v[i])) return (long)i;
    return -1;
}

// the float twin of build_nn2d_i8: constants uploaded as they are ([out_c][kh][kw * in_c] is the filter tensor's own order), finite weights required (a
// zero-padded tap multiplies its weight by 0 where the reference skips it: h_first_non_finite)
static EI_IMPULSE_ERROR build_nn2d_f32(kws_handle *h, size_t &i, int &cur)
{
    const Model &m = h->model;
    KwsNn2dPlanF32 &P = h->nn2df;
    memset(&P, 0, sizeof(P));
    std::vector<H2dBlock> blocks;
    if (EI_IMPULSE_ERROR e = h_nn2d_walk(m, i, cur, true, blocks)) return e;
    P.n_features = (int)m.nn_input_frame_size;
    if (blocks[0].g.in_h * blocks[0].g.in_w * blocks[0].g.in_c != P.n_features)
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "first conv does not consume the feature vector");
    auto floats = [](const Tensor &t) { return std::vector<float>((const float *)t.data.data(), (const float *)t.data.data() + t.data.size() / 4); };
    for (size_t b = 0; b < blocks.size(); b++) {
        const H2dBlock &B = blocks[b];
        const Node &cv = *B.cv;
        const Tensor &w = m.t[cv.in[1]];
        const Tensor *bias = (cv.in.size() > 2 && cv.in[2] >= 0) ? &m.t[cv.in[2]] : nullptr;
        KwsConv2dBlockF32 &k = P.blk[b];
        k.g = B.g;
        const KwsConv2dGeom &g = k.g;
        h_act_range_f32(B.act, &k.conv_min, &k.conv_max);
        h_act_range_f32(B.pool_act, &k.pool_min, &k.pool_max);
        std::vector<float> wv = floats(w), bv((size_t)g.out_c, 0.0f);
        if (wv.size() != (size_t)g.out_c * g.kh * g.krow) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv block %zu: filter size", b);
        if (const long bad = h_first_non_finite(wv); bad >= 0)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv block %zu: weight tensor %d holds a non-finite value (element %ld): the float kernels need finite weights", b,
                        cv.in[1], bad);
        if (bias) { bv = floats(*bias); if (bv.size() != (size_t)g.out_c) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv block %zu: bias size", b); }
        EI_IMPULSE_ERROR e;
        if ((e = h->upload(wv, &k.w))) return e;
        if ((e = h->upload(bv, &k.bias))) return e;
        P.n_blocks++;
    }
    const KwsConv2dGeom &lg = P.blk[P.n_blocks - 1].g;
    P.out_n = lg.pool_h * lg.pool_w * lg.out_c;
    if (kws_nn2d_f32_waves(P) == 0)
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "float 2-D model needs %zu B of LDS at %d waves per workgroup (at most %d): its images do not fit the kernel's LDS budget",
                    kws_nn2d_f32_smem_bytes(P, KWS_NN2D_WAVES_MIN), KWS_NN2D_WAVES_MIN, 150 * 1024);
    h->n_conv2d = P.n_blocks;
    return EI_IMPULSE_OK;
}

// ---- residual graphs ------------------------------------------------------------------------------------------------------------------
// A graph is residual when at least one ADD has two non-constant inputs; every other graph takes the path it always took.
static bool h_is_residual(const Model &m)
{
    for (const Node &nd : m.n)
        if (nd.op == OP_ADD && !m.t[nd.in[0]].is_const && !m.t[nd.in[1]].is_const) return true;
    return false;
}
// A 2-D graph -- the tensor flowing into its first convolution is [1][H][W][C] with H > 1 and W > 1 (h_is_2d's rule) -- that holds a DEPTHWISE_CONV_2D takes
// the step trunks too, ADD or not.  A 1-D graph with depthwise blocks and no tensor + tensor ADD keeps the block kernels.
static bool h_is_dw2d(const Model &m)
{
    bool any_dw = false, first = true, two_d = false;
    for (const Node &nd : m.n) {
        if (nd.op != OP_CONV_2D && nd.op != OP_DEPTHWISE_CONV_2D) continue;
        if (first) {
            const Tensor &x = m.t[nd.in[0]];
            two_d = x.dims.size() == 4 && x.dims[0] == 1 && x.dims[1] > 1 && x.dims[2] > 1;
            first = false;
        }
        any_dw = any_dw || nd.op == OP_DEPTHWISE_CONV_2D;
    }
    return two_d && any_dw;
}

// LDS of the residual trunks at n_waves waves per workgroup, laid out as kws_nnres_trunk_kernel / kws_nnres_f32_trunk_kernel walk it -- per workgroup every
// step's constants, per wave the KWS_RES_SLOTS image slots -- and the wave count their launchers pick (kws_nnres.h)
size_t kws_nnres_smem_bytes(const KwsResPlan &N, int n_waves)
{
    size_t s = 0;
    for (int k = 0; k < N.n_steps; ++k)
        s += N.st[k].g.kind != KWS_RES_ADD ? (((size_t)N.st[k].w_bytes + 15) & ~(size_t)15) + (size_t)N.st[k].g.out_c * 16 : (size_t)KWS_NNRES_ADD_TAB_BYTES;
    return s + (size_t)n_waves * (size_t)N.wave_bytes;
}
int kws_nnres_waves(const KwsResPlan &N)
{
    for (int nw = KWS_NNRES_WAVES_MAX; nw >= KWS_NNRES_WAVES_MIN; --nw)
        if (kws_nnres_smem_bytes(N, nw) <= KWS_NNRES_LDS_I8) return nw;
    return 0;
}
size_t kws_nnres_f32_smem_bytes(const KwsResPlanF32 &N, int n_waves)
{
    size_t s = 0;
    for (int k = 0; k < N.n_steps; ++k) {
        const KwsResGeom &g = N.st[k].g;
        if (g.kind == KWS_RES_ADD) continue;
        s += sizeof(float) * (size_t)((N.st[k].w_lds ? (g.out_c * g.kh * g.krow + 3) & ~3 : 0) + ((g.out_c + 3) & ~3));
    }
    return s + (size_t)n_waves * (size_t)N.wave_bytes;
}
int kws_nnres_f32_waves(const KwsResPlanF32 &N)
{
    for (int nw = KWS_NNRES_WAVES_MAX; nw >= KWS_NNRES_WAVES_MIN; --nw)
        if (kws_nnres_f32_smem_bytes(N, nw) <= KWS_NNRES_LDS_F32) return nw;
    return 0;
}

// one tensor's image: its dims as its convolutions see them, who makes and who last reads it, the margin and extent its consumers need, its slot
struct HResImage {
    int h = 0, w = 0, c = 0, tid = -1;     // tid: a model tensor that carries its quantisation
    int producer = -1, last_use = -1, uses = 0;     // steps (-1: the reshaped input)
    int mt = 0, ml = 0, ext_r = 0, ext_c = 0;       // margin above / left; rows / columns from the tensor's (0, 0) the furthest tap of any consumer reads
    int slot = -1, rows = 0, pitch = 0, bytes = 0, base = 0;
};
struct HResStep { KwsResGeom g; const Node *nd; int a, b, dst, x_id, y_id, act, pool_act, pad_t, pad_l; };
struct HResGraph { std::vector<HResImage> img; std::vector<HResStep> st; int final_img = -1, wave_bytes = 0, n_adds = 0, n_dw = 0; };

// The steps of a residual graph: every node up to the first FULLY_CONNECTED, in node order.  RESHAPEs that keep the quantisation are renamings: a tensor id
// maps to an image and to how its dims spell that image -- as they are ([1][H][W][C]), with H and W exchanged (one of them 1: the same bytes, what Keras'
// Conv1D exports do around their pools), or otherwise (3-D, ...: only another RESHAPE may read it).  Everything comes from an untrusted blob: ids are
// bounds-checked by the parser; here a node may read only the input, constants and outputs of EARLIER nodes, a tensor has one producer, and every dim,
// filter side, stride and pool is bounded BEFORE any arithmetic on it (h_nn2d_walk's manner).  On return i stands at the first FULLY_CONNECTED and cur is
// the flattened tensor it reads.
static EI_IMPULSE_ERROR h_res_walk(const Model &m, size_t &i, int &cur, bool is_float, HResGraph &G)
{
    const uint32_t want = is_float ? TYPE_F32 : TYPE_I8;
    const int elem = is_float ? 4 : 1;
    enum { PLAIN = 0, SWAPPED = 1, OTHER = 2, FLAT_IN = 3 };
    const int nt = (int)m.t.size();
    std::vector<int> img_of(nt, -1), kind_of(nt, OTHER);       // img_of: -1 not produced yet, -2 consumed by a fused pool
    std::vector<char> produced(nt, 0);
    auto quant_ok = [&](int a) {
        const Tensor &t = m.t[a];
        if (t.type != want || t.is_const) return false;
        return is_float || (!t.scale.empty() && !t.zero.empty() && t.zero[0] >= -128 && t.zero[0] <= 127);
    };
    auto same_quant = [&](int a, int b) { return is_float || (m.t[a].scale[0] == m.t[b].scale[0] && m.t[a].zero[0] == m.t[b].zero[0]); };
    auto produce = [&](size_t node, int tid) -> EI_IMPULSE_ERROR {
        if (produced[tid] || m.t[tid].is_const || tid == (int)m.t_in)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "node %zu: tensor %d has a second producer (or is a constant / the input)", node, tid);
        if (!quant_ok(tid)) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "node %zu: output tensor %d: type / quantisation", node, tid);
        produced[tid] = 1;
        return EI_IMPULSE_OK;
    };
    // how dims spell image g: PLAIN, SWAPPED, OTHER (same element count), or -1
    auto spell = [&](const HResImage &g, const std::vector<int> &d) {
        if (d.size() == 4 && d[0] == 1 && d[1] == g.h && d[2] == g.w && d[3] == g.c) return (int)PLAIN;
        if (d.size() == 4 && d[0] == 1 && d[1] == g.w && d[2] == g.h && d[3] == g.c && (g.h == 1 || g.w == 1)) return (int)SWAPPED;
        long n = 1;
        for (int v : d) { if (v < 1 || v > (1 << 24)) return -1; n *= v; if (n > (1l << 28)) return -1; }
        return n == (long)g.h * g.w * g.c ? (int)OTHER : -1;
    };
    auto readable = [&](size_t node, int tid, const char *what) -> EI_IMPULSE_ERROR {
        if (img_of[tid] == -2)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "node %zu: %s tensor %d is the input of a fused MAX_POOL_2D: a pool shares its input with another consumer", node, what, tid);
        if (img_of[tid] < 0 || kind_of[tid] == FLAT_IN)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "node %zu: %s tensor %d is no image an earlier node produced", node, what, tid);
        return EI_IMPULSE_OK;
    };
    if (!quant_ok((int)m.t_in)) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "input tensor type / quantisation");
    produced[m.t_in] = 1; kind_of[m.t_in] = FLAT_IN; img_of[m.t_in] = -3;      // the feature vector: only RESHAPEs read it
    int in_img = -1, flat = -1;
    for (; i < m.n.size(); ++i) {
        const Node &nd = m.n[i];
        if (nd.op == OP_FULLY_CONNECTED) break;
        if (flat >= 0) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "node %zu: only FULLY_CONNECTED layers may follow the flattening RESHAPE", i);
        const int x = nd.in[0], y = nd.out[0];
        if (nd.op == OP_RESHAPE) {
            if (!produced[x] || m.t[x].is_const) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "node %zu: RESHAPE reads tensor %d, which no earlier node produced", i, x);
            if (EI_IMPULSE_ERROR e = produce(i, y)) return e;
            if (!same_quant(x, y)) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "reshape changes quantisation");
            const std::vector<int> &d = m.t[y].dims;
            if (kind_of[x] == FLAT_IN) {
                if (d.size() == 4 && d[0] == 1) {          // the reshaped input: the first image
                    if (d[1] > KWS_NN2D_DIM_MAX || d[2] > KWS_NN2D_DIM_MAX || d[3] > 64 || (size_t)d[1] * d[2] * d[3] != m.nn_input_frame_size)
                        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "node %zu: the input RESHAPE to %d x %d x %d does not hold the %u features (image sides up to %d, 64 channels)",
                                    i, d[1], d[2], d[3], m.nn_input_frame_size, KWS_NN2D_DIM_MAX);
                    if (in_img >= 0) {
                        const int k = spell(G.img[in_img], d);
                        if (k != PLAIN && k != SWAPPED) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "node %zu: a second shape of the input", i);
                        img_of[y] = in_img; kind_of[y] = k;
                        continue;
                    }
                    HResImage g;
                    g.h = d[1]; g.w = d[2]; g.c = d[3]; g.tid = y; g.ext_r = g.h; g.ext_c = g.w;
                    in_img = (int)G.img.size();
                    G.img.push_back(g);
                    img_of[y] = in_img; kind_of[y] = PLAIN;
                } else { img_of[y] = -3; kind_of[y] = FLAT_IN; }
                continue;
            }
            if (EI_IMPULSE_ERROR e = readable(i, x, "RESHAPE input")) return e;
            const HResImage &g = G.img[img_of[x]];
            const int k = spell(g, d);
            if (k < 0) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "node %zu: RESHAPE changes the element count", i);
            img_of[y] = img_of[x]; kind_of[y] = k;
            if (d.size() == 2 && d[0] == 1) { flat = y; G.final_img = img_of[x]; }       // the flatten
            continue;
        }
        if ((int)G.st.size() >= KWS_RES_STEPS_MAX && nd.op != OP_MAX_POOL_2D)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "node %zu: more than %d steps (CONV_2D / ADD) in a residual graph", i, KWS_RES_STEPS_MAX);
        if (nd.op == OP_CONV_2D || nd.op == OP_DEPTHWISE_CONV_2D) {
            const bool dw = nd.op == OP_DEPTHWISE_CONV_2D;
            if (EI_IMPULSE_ERROR e = readable(i, x, "conv input")) return e;
            if (kind_of[x] != PLAIN) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu: its input is a renamed tensor (only MAX_POOL_2D and ADD read those)", i);
            if (EI_IMPULSE_ERROR e = produce(i, y)) return e;
            HResImage &src = G.img[img_of[x]];
            const Tensor &w = m.t[nd.in[1]], &yt = m.t[y];
            const Tensor *bias = (nd.in.size() > 2 && nd.in[2] >= 0) ? &m.t[nd.in[2]] : nullptr;
            if (w.dims.size() != 4 || yt.dims.size() != 4 || yt.dims[0] != 1 || w.type != want)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu: filter and output must be 4-D tensors of the graph's type, one batch", i);
            HResStep S{};
            KwsResGeom &g = S.g;
            g.kind = dw ? KWS_RES_DW : KWS_RES_CONV;
            g.in_c = src.c; g.out_c = w.dims[dw ? 3 : 0]; g.kh = w.dims[1]; g.kw = w.dims[2]; g.dm = 1;
            if (dw) {
                // the filter is [1][kh][kw][in_c * depth_multiplier]; every bound before any product (in_c <= 64: the images' bound)
                g.dm = nd.p[6];
                if (w.dims[0] != 1 || g.dm < 1 || g.dm > 64 || g.out_c < 1 || g.out_c > 64 || g.out_c != g.in_c * g.dm || g.kh < 1 || g.kh > KWS_RES_K_MAX || g.kw < 1 ||
                    g.kw > KWS_RES_K_MAX)
                    return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu: DEPTHWISE_CONV_2D with a [%d][%d][%d][%d] filter and depth multiplier %d over %d channels is not "
                                "served (the filter must be [1][kh][kw][channels x multiplier], multiplier >= 1, sides 1 .. %d, at most 64 output channels)", i,
                                w.dims[0], w.dims[1], w.dims[2], w.dims[3], nd.p[6], g.in_c, KWS_RES_K_MAX);
            } else if (g.out_c > 64 || g.kh > KWS_RES_K_MAX || g.kw > KWS_RES_K_MAX || w.dims[3] != g.in_c)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu: a %d x %d filter over %d (filter: %d) -> %d channels is outside the residual kernels' limits (filter "
                            "sides 1 .. %d, at most 64 channels)", i, g.kh, g.kw, g.in_c, w.dims[3], g.out_c, KWS_RES_K_MAX);
            if (!w.is_const || (bias && (!bias->is_const || bias->type != (is_float ? TYPE_F32 : TYPE_I32) || (long)bias->nbytes != 4l * g.out_c)))
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu: the filter and the bias (%d values, %s) must be constants", i, g.out_c, is_float ? "float32" : "int32");
            const int padding = nd.p[0];
            g.sw = nd.p[1]; g.sh = nd.p[2]; S.act = nd.p[3];
            if (g.sh < 1 || g.sh > KWS_NN2D_STRIDE_MAX || g.sw < 1 || g.sw > KWS_NN2D_STRIDE_MAX)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu: stride %d x %d is outside 1 .. %d", i, g.sh, g.sw, KWS_NN2D_STRIDE_MAX);
            if (nd.p[4] != 1 || nd.p[5] != 1)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu: %sdilation %d x %d: a residual graph's convolutions are not dilated", i,
                            dw ? "DEPTHWISE_CONV_2D with " : "", nd.p[5], nd.p[4]);
            if ((padding != 1 && padding != 2) || S.act < 0 || S.act > 3)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu: padding %d / fused activation %d", i, padding, S.act);
            g.out_h = h_out_size(padding, src.h, g.kh, g.sh, 1); g.out_w = h_out_size(padding, src.w, g.kw, g.sw, 1);
            if (g.out_h < 1 || g.out_w < 1 || yt.dims[1] != g.out_h || yt.dims[2] != g.out_w || yt.dims[3] != g.out_c)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu output shape: the tensor is %d x %d x %d, kernels/padding.h gives %d x %d x %d", i, yt.dims[1], yt.dims[2],
                            yt.dims[3], g.out_h, g.out_w, g.out_c);
            S.pad_t = h_pad_amount(g.sh, 1, src.h, g.kh, g.out_h); S.pad_l = h_pad_amount(g.sw, 1, src.w, g.kw, g.out_w);
            g.krow = dw ? g.kw : g.kw * g.in_c; g.krow4 = (g.krow + 3) & ~3;
            G.n_dw += dw ? 1 : 0;
            src.mt = std::max(src.mt, S.pad_t); src.ml = std::max(src.ml, S.pad_l);
            src.ext_r = std::max(src.ext_r, (g.out_h - 1) * g.sh + g.kh - S.pad_t);
            src.ext_c = std::max(src.ext_c, (g.out_w - 1) * g.sw + g.kw - S.pad_l);
            src.uses++; src.last_use = (int)G.st.size();
            S.nd = &nd; S.a = S.b = img_of[x]; S.x_id = x; S.y_id = y;
            g.ph = g.pw = g.psh = g.psw = 1; g.pool_h = g.out_h; g.pool_w = g.out_w;
            HResImage o;
            o.h = g.out_h; o.w = g.out_w; o.c = g.out_c; o.tid = y; o.ext_r = o.h; o.ext_c = o.w; o.producer = (int)G.st.size();
            S.dst = (int)G.img.size();
            G.img.push_back(o);
            img_of[y] = S.dst; kind_of[y] = PLAIN;
            G.st.push_back(S);
            continue;
        }
        if (nd.op == OP_ADD) {
            const int x2 = nd.in[1];
            if (m.t[x].is_const || m.t[x2].is_const)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "ADD %zu: a constant operand inside a residual graph is not served (its convolutions carry their bias and "
                            "activation)", i);
            if (!produced[x] || !produced[x2]) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "ADD %zu reads a tensor no earlier node produced", i);
            if (EI_IMPULSE_ERROR e = readable(i, x, "ADD operand")) return e;
            if (EI_IMPULSE_ERROR e = readable(i, x2, "ADD operand")) return e;
            const Tensor &ta = m.t[x], &tb = m.t[x2], &to = m.t[y];
            if (ta.dims.size() != 4 || ta.dims != tb.dims || ta.dims != to.dims)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "ADD %zu: its operands and its output must have identical 4-D dims (a broadcasting ADD is not served)", i);
            if (kind_of[x] == OTHER || kind_of[x] != kind_of[x2] || nd.p[0] < 0 || nd.p[0] > 3)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "ADD %zu: operand shapes / fused activation %d", i, nd.p[0]);
            if (EI_IMPULSE_ERROR e = produce(i, y)) return e;
            HResStep S{};
            KwsResGeom &g = S.g;
            HResImage &A = G.img[img_of[x]];
            g.kind = KWS_RES_ADD;
            g.in_c = g.out_c = A.c; g.kh = g.kw = g.sh = g.sw = 1; g.out_h = A.h; g.out_w = A.w;
            g.ph = g.pw = g.psh = g.psw = 1; g.pool_h = g.out_h; g.pool_w = g.out_w;
            S.act = nd.p[0]; S.nd = &nd; S.a = img_of[x]; S.b = img_of[x2]; S.x_id = x; S.y_id = y;
            for (int k : { S.a, S.b }) { G.img[k].uses++; G.img[k].last_use = (int)G.st.size(); }
            HResImage o;
            o.h = g.out_h; o.w = g.out_w; o.c = g.out_c; o.tid = y; o.ext_r = o.h; o.ext_c = o.w; o.producer = (int)G.st.size();
            S.dst = (int)G.img.size();
            G.img.push_back(o);
            img_of[y] = S.dst; kind_of[y] = kind_of[x];
            G.st.push_back(S);
            G.n_adds++;
            continue;
        }
        if (nd.op == OP_MAX_POOL_2D) {
            if (EI_IMPULSE_ERROR e = readable(i, x, "pool input")) return e;
            HResImage &im = G.img[img_of[x]];
            if (im.producer < 0) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool %zu: its input is no step's output (a pool is fused into the step that makes its input)", i);
            HResStep &S = G.st[im.producer];
            KwsResGeom &g = S.g;
            if (im.uses > 0 || g.has_pool)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool %zu: a pool shares its input with another consumer (it is fused into the step that makes its input)", i);
            if (kind_of[x] == OTHER) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool %zu: input shape", i);
            if (EI_IMPULSE_ERROR e = produce(i, y)) return e;
            if (!same_quant(x, y)) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool %zu input", i);
            const bool sw = kind_of[x] == SWAPPED;             // the node's height axis is the image's width
            g.psw = nd.p[sw ? 2 : 1]; g.psh = nd.p[sw ? 1 : 2]; g.pw = nd.p[sw ? 4 : 3]; g.ph = nd.p[sw ? 3 : 4]; S.pool_act = nd.p[5];
            if (g.ph < 1 || g.ph > KWS_NN2D_K_MAX || g.pw < 1 || g.pw > KWS_NN2D_K_MAX || g.psh < 1 || g.psh > KWS_NN2D_K_MAX || g.psw < 1 || g.psw > KWS_NN2D_K_MAX)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool %zu: window %d x %d / stride %d x %d is outside 1 .. %d", i, g.ph, g.pw, g.psh, g.psw, KWS_NN2D_K_MAX);
            if ((nd.p[0] != 1 && nd.p[0] != 2) || S.pool_act < 0 || S.pool_act > 3 || (!is_float && S.pool_act != 0))
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool %zu: padding %d / fused activation %d", i, nd.p[0], S.pool_act);
            g.pool_h = h_out_size(nd.p[0], g.out_h, g.ph, g.psh, 1); g.pool_w = h_out_size(nd.p[0], g.out_w, g.pw, g.psw, 1);
            const std::vector<int> &d = m.t[y].dims;
            if (g.pool_h < 1 || g.pool_w < 1 || d.size() != 4 || d[0] != 1 || d[1] != (sw ? g.pool_w : g.pool_h) || d[2] != (sw ? g.pool_h : g.pool_w) || d[3] != g.out_c)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool %zu output shape: kernels/padding.h gives %d x %d x %d", i, g.pool_h, g.pool_w, g.out_c);
            g.ppt = h_pad_amount(g.psh, 1, g.out_h, g.ph, g.pool_h); g.ppl = h_pad_amount(g.psw, 1, g.out_w, g.pw, g.pool_w);
            if ((g.pool_h - 1) * g.psh - g.ppt >= g.out_h || (g.pool_w - 1) * g.psw - g.ppl >= g.out_w || g.ppt >= g.ph || g.ppl >= g.pw)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool %zu: a window lies outside the image", i);
            g.has_pool = 1;
            for (int t = 0; t < nt; ++t) if (img_of[t] == img_of[x] && t != y) img_of[t] = -2;      // the un-pooled tensor's names: nothing else may read them
            im.h = g.pool_h; im.w = g.pool_w; im.ext_r = im.h; im.ext_c = im.w; im.tid = y;
            img_of[y] = S.dst; kind_of[y] = sw ? SWAPPED : PLAIN;
            continue;
        }
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "node %zu: op %u inside a residual graph", i, nd.op);
    }
    if (i >= m.n.size() || flat < 0 || G.st.empty() || m.n[i].in[0] != flat)
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "expected a flattening RESHAPE and FULLY_CONNECTED after the residual steps");
    cur = flat;
    // the flattened tensor is the LAST step's output and nothing else reads it; every other tensor is read
    if (G.final_img != G.st.back().dst || G.img[G.final_img].uses != 0)
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "the flattened tensor is not the last step's output alone");
    for (size_t k = 0; k < G.img.size(); ++k)
        if ((int)k != G.final_img && G.img[k].uses == 0) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "the output of step %d is never read", G.img[k].producer);
    if ((long)G.img[G.final_img].h * G.img[G.final_img].w * G.img[G.final_img].c > KWS_DENSE_IN_MAX)
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "the residual steps flatten to %ld values: the dense stack takes at most %d inputs",
                    (long)G.img[G.final_img].h * G.img[G.final_img].w * G.img[G.final_img].c, KWS_DENSE_IN_MAX);
    // liveness: at step s the tensors made at or before s (the one being written included) that s or a later step reads
    const int ns = (int)G.st.size();
    int most = 0;
    for (int s = 0; s < ns; ++s) {
        int live = 0;
        for (const HResImage &g : G.img) live += (g.producer <= s && (g.last_use >= s || g.producer == s)) ? 1 : 0;
        most = std::max(most, live);
    }
    if (most > KWS_RES_SLOTS)
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "the residual graph keeps %d tensors live at once (at most %d: a skip connection may span one block)", most, KWS_RES_SLOTS);
    // images and slots: a slot is free for step s's output once its tensor's last reader is before s
    int holder[KWS_RES_SLOTS] = { -1, -1, -1, -1 }, slot_bytes[KWS_RES_SLOTS] = { 0, 0, 0, 0 };
    for (size_t k = 0; k < G.img.size(); ++k) {
        HResImage &g = G.img[k];
        if ((int)k == G.final_img) continue;
        g.rows = g.mt + g.ext_r;
        const int row = (g.ml + g.ext_c) * g.c;
        g.pitch = is_float ? (row | 1) : 4 * (((row + 3) / 4) | 1);             // an odd number of dwords
        const size_t bytes = ((size_t)g.rows * g.pitch * elem + 16 + 15) & ~(size_t)15;
        if (bytes > (size_t)KWS_NNRES_LDS_I8)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "residual model needs %zu B of LDS for one %d x %d x %d image: it does not fit the kernel's LDS budget", bytes, g.h,
                        g.w, g.c);
        g.bytes = (int)bytes;
        for (int s = 0; s < KWS_RES_SLOTS && g.slot < 0; ++s)
            if (holder[s] < 0 || G.img[holder[s]].last_use < g.producer) { g.slot = s; holder[s] = (int)k; }
        if (g.slot < 0) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "the residual graph keeps more than %d tensors live at once", KWS_RES_SLOTS);
        slot_bytes[g.slot] = std::max(slot_bytes[g.slot], g.bytes);
    }
    int base[KWS_RES_SLOTS];
    G.wave_bytes = 0;
    for (int s = 0; s < KWS_RES_SLOTS; ++s) { base[s] = G.wave_bytes / elem; G.wave_bytes += slot_bytes[s]; }
    for (HResImage &g : G.img) if (g.slot >= 0) g.base = base[g.slot];
    for (HResStep &S : G.st) {
        KwsResGeom &g = S.g;
        const HResImage &A = G.img[S.a], &B = G.img[S.b];
        g.a_base = A.base; g.a_pitch = A.pitch; g.a_off = (A.mt - S.pad_t) * A.pitch + (A.ml - S.pad_l) * A.c;
        g.b_base = B.base; g.b_pitch = B.pitch; g.b_off = B.mt * B.pitch + B.ml * B.c;
        const HResImage &D = G.img[S.dst];
        if (S.dst == G.final_img) { g.d_base = -1; g.d_off = 0; g.d_pitch = g.pool_w * g.out_c; g.d_bytes = 0; }
        else { g.d_base = D.base; g.d_off = D.mt * D.pitch + D.ml * D.c; g.d_pitch = D.pitch; g.d_bytes = D.bytes; }
    }
    return EI_IMPULSE_OK;
}

static EI_IMPULSE_ERROR build_nnres_i8(kws_handle *h, size_t &i, int &cur)
{
    const Model &m = h->model;
    KwsResPlan &P = h->nnres;
    memset(&P, 0, sizeof(P));
    HResGraph G;
    if (EI_IMPULSE_ERROR e = h_res_walk(m, i, cur, false, G)) return e;
    const HResImage &in = G.img[0];
    P.n_features = (int)m.nn_input_frame_size;
    P.in_base = in.base; P.in_off = in.mt * in.pitch + in.ml * in.c; P.in_pitch = in.pitch; P.in_bytes = in.bytes; P.in_zp = m.t[in.tid].zero[0];
    P.in_h = in.h; P.in_row = in.w * in.c;
    P.wave_bytes = G.wave_bytes; P.n_adds = G.n_adds; P.n_dw = G.n_dw;
    for (size_t s = 0; s < G.st.size(); s++) {
        const HResStep &S = G.st[s];
        const Node &nd = *S.nd;
        KwsResStep &k = P.st[s];
        k.g = S.g;
        const KwsResGeom &g = k.g;
        const Tensor &y = m.t[S.y_id];
        k.out_zp = y.zero[0]; k.d_zp = y.zero[0];
        h_act_range(S.act, y.scale[0], y.zero[0], &k.act_min, &k.act_max);
        EI_IMPULSE_ERROR e;
        if (g.kind == KWS_RES_DW) {
            // integer_ops/depthwise_conv.h:22-120: weights stay [kh][kw][out_c], bias_eff = bias + input_offset * sum(w[.][.][oc]); the int8 depthwise op clamps
            // to the int8 range and IGNORES its fused activation (depthwise_conv.cc:618-620), as the 1-D kernels do
            const int node_i = (int)(S.nd - &m.n[0]);
            const Tensor &x = m.t[S.x_id], &w = m.t[nd.in[1]];
            const Tensor *bias = (nd.in.size() > 2 && nd.in[2] >= 0) ? &m.t[nd.in[2]] : nullptr;
            const size_t nw = (size_t)g.kh * g.kw * g.out_c;
            std::vector<int8_t> wp((nw + 3) & ~(size_t)3, 0);
            k.w_bytes = (int)wp.size();
            k.act_min = -128; k.act_max = 127;
            std::vector<int32_t> rq((size_t)g.out_c * 4, 0);
            const int32_t *bd = bias ? (const int32_t *)bias->data.data() : nullptr;
            const int32_t in_off = -x.zero[0];
            const bool per_channel = w.scale.size() > 1;
            if (w.data.size() < nw || (bias && bias->data.size() < (size_t)g.out_c * 4))
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %d: DEPTHWISE_CONV_2D constant data", node_i);
            if (w.scale.empty() || (per_channel && ((int)w.scale.size() != g.out_c || w.qdim != 3)))
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %d: DEPTHWISE_CONV_2D per-channel scale count (one scale, or one per output channel along dimension 3)",
                            node_i);
            memcpy(wp.data(), w.data.data(), nw);
            for (int oc = 0; oc < g.out_c; oc++) {
                int64_t wsum = 0, wabs = 0;
                for (int t = 0; t < g.kh * g.kw; t++) { const int v = wp[(size_t)t * g.out_c + oc]; wsum += v; wabs += std::abs(v); }
                rq[(size_t)oc * 4] = (int32_t)((bd ? bd[oc] : 0) + (int64_t)in_off * wsum);
                const double eff = (double)x.scale[0] * (double)(per_channel ? w.scale[oc] : w.scale[0]) / (double)y.scale[0];
                int32_t mult; int sh;
                h_quantize_multiplier(eff, &mult, &sh);          // kernel_util_lite.cc:89-103
                rq[(size_t)oc * 4 + 1] = mult; rq[(size_t)oc * 4 + 2] = sh;
                if (mult < 0 || sh < -31)
                    return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %d: DEPTHWISE_CONV_2D channel %d: requantisation multiplier", node_i, oc);
                if (sh > 0 && h_left_shift_overflows(wabs, in_off, bd ? bd[oc] : 0, sh))
                    return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %d: DEPTHWISE_CONV_2D channel %d: requantisation shifts left by %d and (sum|w| * max|x| + |bias|) "
                                "<< %d can pass 2^31 - 1", node_i, oc, sh, sh);
            }
            if ((e = h->upload(wp, &k.w))) return e;
            if ((e = h->upload(rq, &k.rq))) return e;
        } else if (g.kind == KWS_RES_CONV) {
            // as build_nn2d_i8: weights -> [out_c][kh][krow4], bias_eff = bias + input_offset * sum(w)   (integer_ops/conv.h:64-113)
            const Tensor &x = m.t[S.x_id], &w = m.t[nd.in[1]];
            const Tensor *bias = (nd.in.size() > 2 && nd.in[2] >= 0) ? &m.t[nd.in[2]] : nullptr;
            std::vector<int8_t> wp((size_t)g.out_c * g.kh * g.krow4, 0);
            k.w_bytes = (int)wp.size();
            std::vector<int32_t> rq((size_t)g.out_c * 4, 0);
            const int8_t *wd = (const int8_t *)w.data.data();
            const int32_t *bd = bias ? (const int32_t *)bias->data.data() : nullptr;
            const int32_t in_off = -x.zero[0];
            const bool per_channel = w.scale.size() > 1;
            if (w.data.size() < (size_t)g.out_c * g.kh * g.krow || (bias && bias->data.size() < (size_t)g.out_c * 4))
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv step %zu: constant data", s);
            if (w.scale.empty() || (per_channel && ((int)w.scale.size() != g.out_c || w.qdim != 0)))
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv step %zu: per-channel scale count", s);
            for (int oc = 0; oc < g.out_c; oc++) {
                int64_t wsum = 0, wabs = 0;
                for (int fy = 0; fy < g.kh; fy++)
                    for (int j = 0; j < g.krow; j++) {
                        const int8_t v = wd[((size_t)oc * g.kh + fy) * g.krow + j];
                        wp[((size_t)oc * g.kh + fy) * g.krow4 + j] = v;
                        wsum += v; wabs += std::abs((int)v);
                    }
                rq[(size_t)oc * 4] = (int32_t)((bd ? bd[oc] : 0) + (int64_t)in_off * wsum);
                const double eff = (double)x.scale[0] * (double)(per_channel ? w.scale[oc] : w.scale[0]) / (double)y.scale[0];
                int32_t mult; int sh;
                h_quantize_multiplier(eff, &mult, &sh);          // kernel_util_lite.cc:89-103
                rq[(size_t)oc * 4 + 1] = mult; rq[(size_t)oc * 4 + 2] = sh;
                if (mult < 0 || sh < -31) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv step %zu channel %d: requantisation multiplier", s, oc);
                if (sh > 0 && h_left_shift_overflows(wabs, in_off, bd ? bd[oc] : 0, sh))
                    return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv step %zu channel %d: requantisation shifts left by %d and (sum|w| * max|x| + |bias|) << %d "
                                "can pass 2^31 - 1", s, oc, sh, sh);
            }
            if ((e = h->upload(wp, &k.w))) return e;
            if ((e = h->upload(rq, &k.rq))) return e;
        } else {
            // CalculateOpData, add.cc:271-309; integer_ops/add.h:108-131 per operand value
            const Tensor &t1 = m.t[nd.in[0]], &t2 = m.t[nd.in[1]];
            const int left_shift = 20;
            const double twice_max = 2 * (double)std::max(t1.scale[0], t2.scale[0]);
            const double r1 = (double)t1.scale[0] / twice_max, r2 = (double)t2.scale[0] / twice_max;
            const double ro = twice_max / ((double)(1 << left_shift) * (double)y.scale[0]);
            int32_t m1, m2, mo; int s1, s2, so;
            h_quantize_multiplier(r1, &m1, &s1);
            h_quantize_multiplier(r2, &m2, &s2);
            h_quantize_multiplier(ro, &mo, &so);
            // QuantizeMultiplierSmallerThanOneExp asserts real < 1 and a shift <= 0 (a multiplier that rounds up to 2^31 is halved and shifts by one more)
            if (!(r1 < 1.0) || !(r2 < 1.0) || s1 > 0 || s2 > 0)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "ADD %d: an input multiplier %g / %g is not below 1", (int)(S.nd - &m.n[0]), r1, r2);
            if (!(ro < 1.0) || so > 0)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "ADD %d: the output multiplier 2 max(s1, s2) / (2^20 s_out) = %g is not below 1 (the reference asserts there)",
                            (int)(S.nd - &m.n[0]), ro);
            std::vector<int32_t> tab(512);
            for (int v = -128; v <= 127; v++) {
                tab[v + 128] = h_rdivpot(h_srdhm((v - t1.zero[0]) * (1 << left_shift), m1), -s1);
                tab[256 + v + 128] = h_rdivpot(h_srdhm((v - t2.zero[0]) * (1 << left_shift), m2), -s2);
            }
            k.add_mult = mo; k.add_shift = so;
            if ((e = h->upload(tab, &k.rq))) return e;
        }
        P.tap_bytes += g.pool_h * g.pool_w * g.out_c;
        P.n_steps++;
    }
    const KwsResGeom &lg = P.st[P.n_steps - 1].g;
    P.out_n = lg.pool_h * lg.pool_w * lg.out_c;
    if (kws_nnres_waves(P) == 0)
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "int8 residual model needs %zu B of LDS at %d waves per workgroup (at most %d): it does not fit the kernel's LDS budget",
                    kws_nnres_smem_bytes(P, KWS_NNRES_WAVES_MIN), KWS_NNRES_WAVES_MIN, KWS_NNRES_LDS_I8);
    h->pooled_tap_bytes += P.tap_bytes;
    h->n_res_adds = P.n_adds;
    h->n_res_dw = P.n_dw;
    h->res_trunk = true;
    return EI_IMPULSE_OK;
}

// the float twin of build_nnres_i8: constants as they are, finite weights required (h_first_non_finite).  Filters are staged in LDS while the graph then
// still fits at KWS_NNRES_WAVES_STAGE waves; the largest ones stay in HBM otherwise.
static EI_IMPULSE_ERROR build_nnres_f32(kws_handle *h, size_t &i, int &cur)
{
    const Model &m = h->model;
    KwsResPlanF32 &P = h->nnresf;
    memset(&P, 0, sizeof(P));
    HResGraph G;
    if (EI_IMPULSE_ERROR e = h_res_walk(m, i, cur, true, G)) return e;
    const HResImage &in = G.img[0];
    P.n_features = (int)m.nn_input_frame_size;
    P.in_base = in.base; P.in_off = in.mt * in.pitch + in.ml * in.c; P.in_pitch = in.pitch; P.in_bytes = in.bytes; P.in_h = in.h; P.in_row = in.w * in.c;
    P.wave_bytes = G.wave_bytes; P.n_adds = G.n_adds; P.n_dw = G.n_dw;
    auto floats = [](const Tensor &t) { return std::vector<float>((const float *)t.data.data(), (const float *)t.data.data() + t.data.size() / 4); };
    for (size_t s = 0; s < G.st.size(); s++) {
        const HResStep &S = G.st[s];
        const Node &nd = *S.nd;
        KwsResStepF32 &k = P.st[s];
        k.g = S.g;
        const KwsResGeom &g = k.g;
        h_act_range_f32(S.act, &k.act_min, &k.act_max);
        h_act_range_f32(S.pool_act, &k.pool_min, &k.pool_max);
        P.n_steps++;
        if (g.kind == KWS_RES_ADD) continue;
        // (a depthwise filter [1][kh][kw][out_c] goes as it is too: krow = kw, the same out_c * kh * krow values)
        const Tensor &w = m.t[nd.in[1]];
        const Tensor *bias = (nd.in.size() > 2 && nd.in[2] >= 0) ? &m.t[nd.in[2]] : nullptr;
        std::vector<float> wv = floats(w), bv((size_t)g.out_c, 0.0f);
        if (wv.size() != (size_t)g.out_c * g.kh * g.krow) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv step %zu: filter size", s);
        if (const long bad = h_first_non_finite(wv); bad >= 0 && g.kind == KWS_RES_DW)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %d: DEPTHWISE_CONV_2D weight tensor %d holds a non-finite value (element %ld): the float kernels need "
                        "finite weights", (int)(S.nd - &m.n[0]), nd.in[1], bad);
        else if (bad >= 0)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv step %zu: weight tensor %d holds a non-finite value (element %ld): the float kernels need finite weights", s,
                        nd.in[1], bad);
        if (bias) { bv = floats(*bias); if (bv.size() != (size_t)g.out_c) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv step %zu: bias size", s); }
        k.w_lds = 1;
        EI_IMPULSE_ERROR e;
        if ((e = h->upload(wv, &k.w))) return e;
        if ((e = h->upload(bv, &k.bias))) return e;
    }
    const KwsResGeom &lg = P.st[P.n_steps - 1].g;
    P.out_n = lg.pool_h * lg.pool_w * lg.out_c;
    while (kws_nnres_f32_smem_bytes(P, KWS_NNRES_WAVES_STAGE) > KWS_NNRES_LDS_F32) {                 // the largest staged filter goes back to HBM
        int big = -1;
        for (int s = 0; s < P.n_steps; ++s)
            if (P.st[s].g.kind != KWS_RES_ADD && P.st[s].w_lds &&
                (big < 0 || P.st[s].g.out_c * P.st[s].g.kh * P.st[s].g.krow > P.st[big].g.out_c * P.st[big].g.kh * P.st[big].g.krow)) big = s;
        if (big < 0) break;                               // (the images alone: fewer waves, down to KWS_NNRES_WAVES_MIN)
        P.st[big].w_lds = 0;
    }
    if (kws_nnres_f32_waves(P) == 0)
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "float residual model needs %zu B of LDS at %d waves per workgroup (at most %d): its images do not fit the kernel's "
                    "LDS budget", kws_nnres_f32_smem_bytes(P, KWS_NNRES_WAVES_MIN), KWS_NNRES_WAVES_MIN, KWS_NNRES_LDS_F32);
    h->n_res_adds = P.n_adds;
    h->n_res_dw = P.n_dw;
    h->res_trunk = true;
    return EI_IMPULSE_OK;
}

static EI_IMPULSE_ERROR build_nn_plan_f32(kws_handle *h)
{
    const Model &m = h->model;
    KwsNnPlanF32 &N = h->nnf;
    memset(&N, 0, sizeof(N));
    h->is_float = true;
    memset(&h->nn, 0, sizeof(h->nn));
    h->nn.in_scale = 1.0f;                               // never used for a result: float models have no int8 input tensor
    h->nn.n_features = (int)m.nn_input_frame_size;
    N.n_features = (int)m.nn_input_frame_size;
    N.n_labels = (int)m.labels.size();
    for (const Tensor &t : m.t)
        if (t.type != TYPE_F32 && !(t.type == TYPE_I32 && t.is_const))     // int32 constants: RESHAPE shape operands
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "mixed float/integer graphs are not implemented");

    int cur = (int)m.t_in, cur_w = 0, cur_c = 0;
    size_t i = 0;
    auto skip_reshapes = [&]() {
        while (i < m.n.size() && m.n[i].op == OP_RESHAPE && m.n[i].in[0] == cur) { cur = m.n[i].out[0]; i++; }
    };
    auto floats = [](const Tensor &t) { return std::vector<float>((const float *)t.data.data(), (const float *)t.data.data() + t.nbytes / 4); };
    // a residual graph: its steps in a plan of their own (this one keeps n_blocks = 0), then the dense stack -- always
    int inputs2d = 0;
    const bool residual = h_is_residual(m) || h_is_dw2d(m);        // (a 2-D graph with depthwise steps takes the step trunks too)
    if (residual) {
        if (EI_IMPULSE_ERROR e = build_nnres_f32(h, i, cur)) return e;
        inputs2d = h->nnresf.out_n;
    }
    skip_reshapes();
    // a 2-D graph: its blocks in a plan of their own (this one keeps n_blocks = 0), then the dense stack -- always, a single FULLY_CONNECTED included
    if (!residual && h_is_2d(m, i, cur)) {
        if (EI_IMPULSE_ERROR e = build_nn2d_f32(h, i, cur)) return e;
        if (i >= m.n.size() || m.n[i].op != OP_FULLY_CONNECTED) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "expected FULLY_CONNECTED after the conv blocks");
        inputs2d = h->nn2df.out_n;
    }
    while (i < m.n.size() && (m.n[i].op == OP_CONV_2D || m.n[i].op == OP_DEPTHWISE_CONV_2D)) {
        if (N.n_blocks >= KWS_MAX_BLOCKS) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "more than %d conv blocks", KWS_MAX_BLOCKS);
        const Node &cv = m.n[i];
        const bool dw = cv.op == OP_DEPTHWISE_CONV_2D;
        if (cv.in[0] != cur || cv.in.size() < 2) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv input is not the flowing tensor");
        const Tensor &x = m.t[cur], &w = m.t[cv.in[1]], &y = m.t[cv.out[0]];
        const Tensor *bias = (cv.in.size() > 2 && cv.in[2] >= 0) ? &m.t[cv.in[2]] : nullptr;
        const int in_h = x.dim4(1), in_w = x.dim4(2), in_c = x.dim4(3);
        const int out_c = dw ? w.dim4(3) : w.dim4(0), f_h = w.dim4(1), f_w = w.dim4(2);
        const int depth_mult = dw ? cv.p[6] : 1;
        const int padding = cv.p[0], stride_w = cv.p[1], stride_h = cv.p[2], act = cv.p[3], dil_w = cv.p[4], dil_h = cv.p[5];
        if (x.dim4(0) != 1 || in_h != 1 || f_h != 1 || !w.is_const ||
            (dw ? (w.dim4(0) != 1 || depth_mult < 1 || out_c != in_c * depth_mult) : (w.dim4(3) != in_c)) || (bias && !bias->is_const) ||
            f_w > 16 || out_c > 64 || x.dims.size() != 4 || (size_t)w.nbytes != sizeof(float) * out_c * f_w * (dw ? 1 : in_c))
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu is not a 1xK (depthwise) convolution over time", i);
        if (const char *why = h_conv_geometry_why(dw, padding, in_w, f_w, stride_w, stride_h, dil_w, dil_h))
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu: %s (stride %d x %d, dilation %d x %d)", i, why, stride_w, stride_h, dil_w, dil_h);
        if (cur_w && (cur_w != in_w || cur_c != in_c)) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "shape mismatch into conv %zu", i);
        const int out_w = h_out_size(padding, in_w, f_w, stride_w, dil_w);         // padding.h with the real stride and dilation; a negative total padding is 0
        const int pad_left = h_pad_amount(stride_w, dil_w, in_w, f_w, out_w);
        if (out_w < 1 || out_w != y.dim4(2) || y.dim4(3) != out_c)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu output shape: the tensor has %d rows, stride %d and dilation %d give %d", i, y.dim4(2), stride_w, dil_w, out_w);
        KwsConvBlockF32 &k = N.blk[N.n_blocks];
        k.in_w = in_w; k.in_c = in_c; k.out_c = out_c; k.taps = f_w; k.pad_left = pad_left; k.out_w = out_w;
        k.stride = (short)stride_w; k.dilation = (short)dil_w;         // (both below KWS_NN_IMAGE_MAX: h_conv_geometry_why)
        k.depthwise = dw ? 1 : 0; k.depth_mult = depth_mult;
        h_act_range_f32(act, &k.conv_min, &k.conv_max);           // the float depthwise op honours its activation
        std::vector<float> wv = floats(w), bv(out_c, 0.0f), av(out_c, 0.0f);
        if ((int)wv.size() != out_c * f_w * (dw ? 1 : in_c)) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu filter size", i);
        if (const long bad = h_first_non_finite(wv); bad >= 0)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu: weight tensor %d holds a non-finite value (element %ld): the float kernels need finite weights", i,
                        cv.in[1], bad);
        if (bias) { if ((int)bias->nbytes != out_c * 4) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv %zu bias size", i); bv = floats(*bias); }
        cur = cv.out[0]; cur_w = out_w; cur_c = out_c;
        i++;
        skip_reshapes();
        k.has_add = 0;
        h_act_range_f32(0, &k.add_min, &k.add_max);
        if (i < m.n.size() && m.n[i].op == OP_ADD) {
            const Node &ad = m.n[i];
            int a_id = ad.in[0], b_id = ad.in[1];
            if (a_id != cur && b_id == cur) std::swap(a_id, b_id);
            const Tensor &cb = m.t[b_id];
            if (a_id != cur || !cb.is_const || (int)cb.nbytes != out_c * 4 || cb.dims.back() != out_c)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "ADD %zu is not a per-channel constant add", i);
            av = floats(cb);                              // x + c == c + x in IEEE arithmetic: operand order is immaterial
            k.has_add = 1;
            h_act_range_f32(ad.p[0], &k.add_min, &k.add_max);
            cur = ad.out[0];
            i++;
            skip_reshapes();
        }
        k.pool = 1; k.pool_stride = 1; k.pool_w = out_w;
        h_act_range_f32(0, &k.pool_min, &k.pool_max);
        if (i < m.n.size() && m.n[i].op == OP_MAX_POOL_2D) {
            const Node &pl = m.n[i];
            const Tensor &px = m.t[pl.in[0]], &py = m.t[pl.out[0]];
            if (pl.in[0] != cur) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool %zu input", i);
            const int ph = px.dim4(1), pw = px.dim4(2);
            int f, s, out_n;
            if (pw == 1 && ph == cur_w) { f = pl.p[4]; s = pl.p[2]; if (pl.p[3] != 1) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "2-D pool"); out_n = py.dim4(1); }
            else if (ph == 1 && pw == cur_w) { f = pl.p[3]; s = pl.p[1]; if (pl.p[4] != 1) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "2-D pool"); out_n = py.dim4(2); }
            else return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool %zu is not over the time axis", i);
            const int po = h_out_size(pl.p[0], cur_w, f, s, 1);
            if (po != out_n || h_pad_amount(s, 1, cur_w, f, po) != 0 || (po - 1) * s >= cur_w || f > 8)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "pool %zu window/padding outside the kernel's limits", i);
            k.pool = f; k.pool_stride = s; k.pool_w = po;
            h_act_range_f32(pl.p[5], &k.pool_min, &k.pool_max);
            cur = pl.out[0]; cur_w = po;
            i++;
            skip_reshapes();
        }
        EI_IMPULSE_ERROR e;
        if ((e = h->upload(wv, &k.w))) return e;
        if ((e = h->upload(bv, &k.bias))) return e;
        if ((e = h->upload(av, &k.addc))) return e;
        h->hostf.w[N.n_blocks] = wv; h->hostf.bias[N.n_blocks] = bv; h->hostf.addc[N.n_blocks] = av;
        kws_nn_f32_pick_blocking(&k);
        N.n_blocks++;
    }
    if (N.n_blocks > 0 && N.blk[0].in_w * N.blk[0].in_c != N.n_features) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "first conv does not consume the feature vector");
    for (int b = 0; b + 1 < N.n_blocks; b++)
        if (N.blk[b].pool_w != N.blk[b + 1].in_w || N.blk[b].out_c != N.blk[b + 1].in_c)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "conv blocks do not chain");
    if (h_dense_stack(m, i, N.n_blocks)) {
        // dense stack: fully_connected.h:26-60 per layer, in the reference's order
        KwsDensePlanF32 &D = h->densef;
        memset(&D, 0, sizeof(D));
        D.n_labels = N.n_labels;
        const int inputs = inputs2d ? inputs2d : N.n_blocks ? N.blk[N.n_blocks - 1].pool_w * N.blk[N.n_blocks - 1].out_c : N.n_features;
        int k_in = inputs;
        while (i < m.n.size() && m.n[i].op == OP_FULLY_CONNECTED) {
            const int li = D.n_layers;
            if (li >= KWS_DENSE_MAX) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "more than %d FULLY_CONNECTED layers", KWS_DENSE_MAX);
            const Node &fc = m.n[i];
            if (fc.in[0] != cur) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "dense layer %d: input is not the flowing tensor", li);
            const Tensor &w = m.t[fc.in[1]], &y = m.t[fc.out[0]];
            const Tensor *bias = (fc.in.size() > 2 && fc.in[2] >= 0) ? &m.t[fc.in[2]] : nullptr;
            const long units = w.dims[0], k = w.dims[1];
            if (w.type != TYPE_F32 || y.type != TYPE_F32 || m.t[cur].type != TYPE_F32)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "dense layer %d: tensor types", li);
            if (k != k_in || k > KWS_DENSE_IN_MAX || units < 1 || units > KWS_DENSE_UNITS_MAX || units * k * 4 > KWS_DENSE_W_MAX * 4l || !w.is_const ||
                (long)w.nbytes != units * k * 4 || (long)w.data.size() < units * k * 4 || y.dims.back() != units || (long)y.nbytes != units * 4)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "dense layer %d: weights [%ld][%ld] for %d inputs are outside the kernel's limits (%d units, %d inputs, %d weights)",
                            li, units, k, k_in, KWS_DENSE_UNITS_MAX, KWS_DENSE_IN_MAX, KWS_DENSE_W_MAX);
            if (bias && (!bias->is_const || bias->type != TYPE_F32 || (long)bias->nbytes != units * 4 || (long)bias->data.size() < units * 4))
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "dense layer %d: bias", li);
            if (fc.p[0] < 0 || fc.p[0] > 3) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "dense layer %d: fused activation %d", li, fc.p[0]);
            KwsDenseLayerF32 &L = D.l[li];
            L.k = (int)k; L.units = (int)units;
            h_act_range_f32(fc.p[0], &L.lo, &L.hi);
            std::vector<float> wv = floats(w), bv((size_t)units, 0.0f);
            if (const long bad = h_first_non_finite(wv); bad >= 0)
                return fail(KWS_ERROR_UNSUPPORTED_MODEL, "dense layer %d: weight tensor %d holds a non-finite value (element %ld): the float kernels need finite weights",
                            li, fc.in[1], bad);
            if (bias) bv = floats(*bias);
            EI_IMPULSE_ERROR e;
            if ((e = h->upload(wv, &L.w))) return e;
            if ((e = h->upload(bv, &L.bias))) return e;
            D.buf_floats[li & 1] = std::max(D.buf_floats[li & 1], L.units);
            D.n_layers++;
            cur = fc.out[0];
            k_in = L.units;
            i++;
            skip_reshapes();
        }
        const KwsDenseLayerF32 &last = D.l[D.n_layers - 1];
        if (last.units != N.n_labels || last.units > 48)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "the last FULLY_CONNECTED has %d outputs for %d labels (at most 48)", last.units, N.n_labels);
        if (i >= m.n.size() || m.n[i].op != OP_SOFTMAX || m.n[i].in[0] != cur || m.n[i].out[0] != (int)m.t_out || i + 1 != m.n.size())
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "expected a final SOFTMAX");
        N.beta = D.beta = m.n[i].beta;
        N.fc_in = inputs; N.fc_out = 0;                  // the trunk form of kws_nn_f32_kernel sizes its output vector by fc_in; it has no head
        N.dense = &D; N.handoff = &h->handoff;
        handoff_init(h, sizeof(float) * (size_t)inputs);
        if (residual) h->handoff.trunkres_f32 = &h->nnresf;
        else if (inputs2d) h->handoff.trunk2d_f32 = &h->nn2df;
        h->n_dense = D.n_layers;
        if (N.n_blocks > 0 && kws_nn_f32_smem_bytes(N, 4) > 150 * 1024) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "float model too large for the kernel's LDS budget");
        void *d = nullptr;
        HIP_TRY(hipMalloc(&d, sizeof(KwsNnPlanF32)));
        h->dev_allocs.push_back(d);
        HIP_TRY(hipMemcpy(d, &N, sizeof(KwsNnPlanF32), hipMemcpyHostToDevice));
        h->d_nnf = (const KwsNnPlanF32 *)d;
        return EI_IMPULSE_OK;
    }
    if (N.n_blocks == 0) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "graph does not start with a convolution block");
    if (i >= m.n.size() || m.n[i].op != OP_FULLY_CONNECTED || m.n[i].in[0] != cur)
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "expected FULLY_CONNECTED after the conv blocks");
    {
        const Node &fc = m.n[i];
        const Tensor &w = m.t[fc.in[1]];
        const Tensor *bias = (fc.in.size() > 2 && fc.in[2] >= 0) ? &m.t[fc.in[2]] : nullptr;
        N.fc_in = w.dims.back(); N.fc_out = w.dims[0];
        const KwsConvBlockF32 &lb = N.blk[N.n_blocks - 1];
        if (N.fc_in != lb.pool_w * lb.out_c || N.fc_in > KWS_FC_IN_MAX || N.fc_in * N.fc_out * 4 > KWS_FC_W_MAX || N.fc_out > 48 || N.fc_out != N.n_labels || !w.is_const ||
            (int)w.nbytes != N.fc_in * N.fc_out * 4)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "FULLY_CONNECTED shape %dx%d outside the kernel's limits", N.fc_out, N.fc_in);
        h_act_range_f32(fc.p[0], &N.fc_min, &N.fc_max);
        std::vector<float> wv = floats(w), bv(N.fc_out, 0.0f);
        if (const long bad = h_first_non_finite(wv); bad >= 0)
            return fail(KWS_ERROR_UNSUPPORTED_MODEL, "FULLY_CONNECTED: weight tensor %d holds a non-finite value (element %ld): the float kernels need finite weights",
                        fc.in[1], bad);
        if (bias) { if ((int)bias->nbytes != N.fc_out * 4) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "FULLY_CONNECTED bias size"); bv = floats(*bias); }
        EI_IMPULSE_ERROR e;
        if ((e = h->upload(wv, &N.fc_w))) return e;
        if ((e = h->upload(bv, &N.fc_bias))) return e;
        h->hostf.fc_w = wv; h->hostf.fc_b = bv;
        cur = fc.out[0];
        i++;
    }
    if (i >= m.n.size() || m.n[i].op != OP_SOFTMAX || m.n[i].in[0] != cur || m.n[i].out[0] != (int)m.t_out || i + 1 != m.n.size())
        return fail(KWS_ERROR_UNSUPPORTED_MODEL, "expected a final SOFTMAX");
    N.beta = m.n[i].beta;
    if (kws_nn_f32_smem_bytes(N, 4) > 150 * 1024) return fail(KWS_ERROR_UNSUPPORTED_MODEL, "float model too large for the kernel's LDS budget");
    {
        void *d = nullptr;
        HIP_TRY(hipMalloc(&d, sizeof(KwsNnPlanF32)));
        h->dev_allocs.push_back(d);
        HIP_TRY(hipMemcpy(d, &N, sizeof(KwsNnPlanF32), hipMemcpyHostToDevice));
        h->d_nnf = (const KwsNnPlanF32 *)d;
    }
    return EI_IMPULSE_OK;
}

