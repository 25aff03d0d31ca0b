// Stand-alone device program: csrc/kws_fast_maxmin.h -- the fast kernel's single-instruction maximum / minimum helpers -- against fmaxf / fminf as the
// compiler builds them, on the GPU, bit for bit: every pairing of a table of specials (zeros of either sign, subnormals, infinities, quiet NaNs with and
// without a payload, the largest and smallest normal numbers) with itself and with random bit patterns, and a few thousand random pairs.  Signalling NaNs
// are left out (the helpers' contract: no arithmetic of the kernel produces one); a random pattern that is one gets its quiet bit set.  Two NaN results
// count as equal: payloads are not part of the claim.
//
//     fast_maxmin_driver            ->  "CASES <n> MISMATCH <m>" (and the first few mismatches)
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "kws_fast_maxmin.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

__device__ __forceinline__ bool same(float x, float y)
{
    return __float_as_uint(x) == __float_as_uint(y) || (x != x && y != y);
}

// thread i: a = A[i] against every b = B[j] (j wave-uniform, so the _u helpers receive their bound in a scalar register, as in the kernel)
__global__ void maxmin_kernel(const float *__restrict__ A, int na, const float *__restrict__ B, int nb, unsigned long long *__restrict__ bad, unsigned *__restrict__ first)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const float a = A[i < na ? i : na - 1];
    for (int j = 0; j < nb; ++j) {
        const float b = B[j];
        const float bu = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, b)));
        unsigned m = 0;
        m |= same(fast_max(a, b), fmaxf(a, b)) ? 0 : 1;
        m |= same(fast_min(a, b), fminf(a, b)) ? 0 : 2;
        m |= same(fast_max(b, a), fmaxf(b, a)) ? 0 : 4;
        m |= same(fast_min(b, a), fminf(b, a)) ? 0 : 8;
        m |= same(fast_max_u(a, bu), fmaxf(a, b)) ? 0 : 16;
        m |= same(fast_min_u(a, bu), fminf(a, b)) ? 0 : 32;
        m |= same(fast_max_abs(a, b), fmaxf(fabsf(a), fabsf(b))) ? 0 : 64;
        // the clamps as the kernel chains them: (v, lo, hi) = (a, b, |b|) and (a, -|b|, b)
        const float hb = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, fabsf(b))));
        const float lb = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, -fabsf(b))));
        m |= same(fast_clamp_u(a, bu, hb), fminf(fmaxf(a, b), fabsf(b))) ? 0 : 128;
        m |= same(fast_clamp_u(a, lb, bu), fminf(fmaxf(a, -fabsf(b)), b)) ? 0 : 256;
        if (m != 0 && i < na) {
            const unsigned long long k = atomicAdd(bad, 1ull);
            if (k < 8) { first[3 * k] = __float_as_uint(a); first[3 * k + 1] = __float_as_uint(b); first[3 * k + 2] = m; }
        }
    }
}

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, sizeof f); return f; }

int main()
{
    const uint32_t specials[] = {
        0x00000000u, 0x80000000u,                               // +-0
        0x00000001u, 0x80000001u, 0x007fffffu, 0x807fffffu, 0x00400000u, 0x80400000u,       // subnormals: smallest, largest, one in between
        0x00800000u, 0x80800000u, 0x7f7fffffu, 0xff7fffffu,     // smallest / largest normal numbers
        0x7f800000u, 0xff800000u,                               // +-inf
        0x7fc00000u, 0xffc00000u, 0x7fc12345u, 0xffffffffu,     // quiet NaNs: default, negative, with payloads
        0x3f800000u, 0xbf800000u, 0x3f800001u, 0xbf800001u, 0x40c00000u, 0xc0c00000u, 0x33800000u, 0xb3800000u };
    std::vector<float> A, B;
    for (uint32_t u : specials) { A.push_back(from_bits(u)); B.push_back(from_bits(u)); }
    uint64_t s = 0x9e3779b97f4a7c15ull;
    auto rnd = [&]() {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        uint32_t u = (uint32_t)(s >> 16);
        if ((u & 0x7f800000u) == 0x7f800000u && (u & 0x007fffffu) != 0) u |= 0x00400000u;      // a NaN: quiet
        return from_bits(u);
    };
    for (int i = 0; i < 4096; ++i) A.push_back(rnd());
    for (int i = 0; i < 64; ++i) B.push_back(rnd());
    const int na = (int)A.size(), nb = (int)B.size();
    float *dA, *dB;
    unsigned long long *dbad, bad = 0;
    unsigned *dfirst, first[24] = { 0 };
    CHECK(hipMalloc(&dA, na * sizeof(float)));
    CHECK(hipMalloc(&dB, nb * sizeof(float)));
    CHECK(hipMalloc(&dbad, sizeof bad));
    CHECK(hipMalloc(&dfirst, sizeof first));
    CHECK(hipMemcpy(dA, A.data(), na * sizeof(float), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dB, B.data(), nb * sizeof(float), hipMemcpyHostToDevice));
    CHECK(hipMemset(dbad, 0, sizeof bad));
    CHECK(hipMemset(dfirst, 0, sizeof first));
    maxmin_kernel<<<(na + 255) / 256, 256>>>(dA, na, dB, nb, dbad, dfirst);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(&bad, dbad, sizeof bad, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(first, dfirst, sizeof first, hipMemcpyDeviceToHost));
    for (unsigned long long k = 0; k < bad && k < 8; ++k) printf("BAD a %08x b %08x helpers %03x\n", first[3 * k], first[3 * k + 1], first[3 * k + 2]);
    printf("CASES %lld MISMATCH %llu\n", 9ll * na * nb, bad);
    (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dbad); (void)hipFree(dfirst);
    return 0;
}
