// general_dsp_host_driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_general_envelope_host.py): which MFCC plans kws_create admits over the
// shapes of tests/general_dsp_shapes.py and which kernels a batch call then launches, against the launch-recording stub HIP runtime of
// tests/ragged/ragged_hip_stub.cpp (device memory = host heap, launches do nothing) under ASan + UBSan.  No value a kernel would write means
// anything here.  The stub logs a launch under the kernel's mangled name, so the build of the cooperative kernel (its template arguments:
// float input, frames per chunk, waves per SIMD, pair loads) can be told from the name.
// usage: kws_general_dsp_san <blob> ...      prints per blob
//   load <n> <code> <kws_mfcc_kernel_name or the refusal's text>
//   route <n> <call> <code> <tuned mfcc8> <cooperative> <two-wave build> <four-wave build> <with pair loads> <scratch> <fused tuned cmvnw + network> <cmvnw lds> <cmvnw global> <all launches>
//   fast <n> <code> <kws_last_error text>
//   done
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/kws/kws.h"

extern "C" void kws_stub_launch_reset(void);
extern "C" int kws_stub_launch_count(const char *substring);

// launches of kws_spectral_lds_kernel<F32IN, LCH, WPS, PK> with the given waves per SIMD (0: any) and pair loads (-1: either)
static int coop(int wps, int pk)
{
    int n = 0;
    for (int f32 = 0; f32 < 2; f32++)
        for (int lch = 4; lch <= 8; lch += 4)
            for (int w = 2; w <= 4; w += 2)
                for (int k = 0; k < 2; k++) {
                    if ((wps && w != wps) || (pk >= 0 && k != pk)) continue;
                    char name[96];
                    snprintf(name, sizeof(name), "kws_spectral_lds_kernelILb%dELi%dELi%dELb%dEE", f32, lch, w, k);
                    n += kws_stub_launch_count(name);
                }
    return n;
}

static void route(int mi, const char *call, EI_IMPULSE_ERROR rc)
{
    printf("route %d %s %d %d %d %d %d %d %d %d %d %d %d\n", mi, call, (int)rc, kws_stub_launch_count("kws_mfcc8_kernel"), kws_stub_launch_count("kws_spectral_lds_kernel"),
           coop(2, -1), coop(4, -1), coop(0, 1), kws_stub_launch_count("kws_spectral_generic_kernel"), kws_stub_launch_count("kws_cmvn_nn_kernel"),
           kws_stub_launch_count("kws_cmvn_lds_kernel"), kws_stub_launch_count("kws_cmvn_generic_kernel"), kws_stub_launch_count(""));
}

int main(int argc, char **argv)
{
    for (int mi = 0; mi + 1 < argc; mi++) {
        FILE *fp = fopen(argv[mi + 1], "rb");
        if (!fp) return 2;
        std::vector<unsigned char> blob;
        unsigned char buf[4096];
        for (size_t n; (n = fread(buf, 1, sizeof(buf), fp)) > 0;) blob.insert(blob.end(), buf, buf + n);
        fclose(fp);
        kws_handle *h = nullptr;
        const EI_IMPULSE_ERROR rc = kws_create(blob.data(), blob.size(), 0, &h);
        printf("load %d %d %s\n", mi, (int)rc, rc ? kws_last_error() : kws_mfcc_kernel_name(h));
        if (rc) continue;
        const size_t B = 5, clip = (size_t)kws_clip_samples(h), F = (size_t)kws_feature_count(h);
        int16_t *pcm = (int16_t *)aligned_alloc(64, (B * clip * sizeof(int16_t) + 63) & ~(size_t)63);
        for (size_t i = 0; i < B * clip; i++) pcm[i] = (int16_t)(i * 37u % 2001u) - 1000;
        std::vector<float> s(B * (size_t)kws_label_count(h)), f(B * F), f2(B * F);
        std::vector<int8_t> q(B * F);
        kws_stub_launch_reset();
        route(mi, "classify", kws_run_classifier_batch_device(h, pcm, B, s.data(), f.data(), q.data(), nullptr));
        kws_stub_launch_reset();
        route(mi, "extract_mfcc", kws_extract_mfcc_batch_device(h, pcm, B, f.data(), nullptr, nullptr));
        kws_stub_launch_reset();
        route(mi, "mfcc", kws_mfcc_batch_device(h, pcm, B, f.data(), nullptr));
        kws_stub_launch_reset();
        route(mi, "cmvn_inference", kws_cmvn_inference_batch_device(h, f.data(), B, s.data(), f2.data(), nullptr, nullptr));
        const EI_IMPULSE_ERROR rf = kws_set_mode(h, KWS_MODE_FAST);
        printf("fast %d %d %s\n", mi, (int)rf, rf ? kws_last_error() : "");
        free(pcm);
        kws_destroy(h);
    }
    printf("done\n");
    return 0;
}
