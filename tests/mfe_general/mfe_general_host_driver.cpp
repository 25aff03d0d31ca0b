// mfe_general_host_driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_mfe_general_host.py): which plans kws_create admits for MFE-block models
// and which kernels a batch call then launches, against the launch-recording stub HIP runtime of tests/ragged/ragged_hip_stub.cpp (device
// memory = host heap, launches do nothing) under ASan + UBSan.  No value a kernel would write means anything here.
// usage: kws_mfe_general_san <blob> ...      prints per blob
//   load <n> <code> <kws_mfcc_kernel_name or the refusal's text>
//   route <n> <call> <code> <tuned mfcc8> <tuned mfcc> <cooperative> <scratch> <tuned norm> <lds norm> <centre> <scale> <quantise> <unring> <all launches>
//   fast <n> <code> <kws_last_error text>
//   done
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/kws/kws.h"

extern "C" void kws_stub_launch_reset(void);
extern "C" int kws_stub_launch_count(const char *substring);

static void route(int mi, const char *call, EI_IMPULSE_ERROR rc)
{
    printf("route %d %s %d %d %d %d %d %d %d %d %d %d %d %d\n", mi, call, (int)rc, kws_stub_launch_count("kws_mfcc8_kernel"),
           kws_stub_launch_count("kws_mfcc_kernel"), kws_stub_launch_count("kws_spectral_lds_kernel"), kws_stub_launch_count("kws_spectral_generic_kernel"),
           kws_stub_launch_count("kws_mfe_norm_kernel"), kws_stub_launch_count("kws_mfe_norm_lds_kernel"), kws_stub_launch_count("kws_mfe_center_generic_kernel"),
           kws_stub_launch_count("kws_mfe_scale_generic_kernel"), kws_stub_launch_count("kws_quantize_kernel"), kws_stub_launch_count("kws_unring_kernel"),
           kws_stub_launch_count(""));
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
        const bool is_float = kws_model_is_float(h) != 0;
        kws_stub_launch_reset();
        route(mi, "classify", kws_run_classifier_batch_device(h, pcm, B, s.data(), f.data(), is_float ? nullptr : q.data(), nullptr));
        kws_stub_launch_reset();
        route(mi, "classify_unaligned", kws_run_classifier_batch_device(h, pcm + 1, B - 1, s.data(), f.data(), nullptr, nullptr));
        kws_stub_launch_reset();
        route(mi, "extract_mfe", kws_extract_mfe_batch_device(h, pcm, B, f.data(), nullptr));
        kws_stub_launch_reset();
        route(mi, "mfe", kws_mfe_batch_device(h, pcm, B, f.data(), nullptr, nullptr));
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
