// ragged_hip_stub.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_ragged_host.py).  The stand-in HIP runtime of tests/sanitize/hip_stub.cpp
// (device memory is host heap, kernel launches do nothing and report success: no arithmetic of the product runs here) which also RECORDS
// launches: every kernel registers under its name when the program starts, and a launch is logged under that name, so that a test can say
// how many launches of which kernels a call made -- or that it made none.
//   kws_stub_launch_reset()            forget the log
//   kws_stub_launch_count(substring)   launches since then whose kernel name contains the substring ("" counts all)
#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

static std::map<const void *, std::string> &stub_names() { static std::map<const void *, std::string> m; return m; }
static std::vector<std::string> &stub_log() { static std::vector<std::string> v; return v; }

extern "C" {
void kws_stub_launch_reset(void) { stub_log().clear(); }
int kws_stub_launch_count(const char *substring)
{
    int n = 0;
    for (const std::string &s : stub_log()) if (s.find(substring) != std::string::npos) ++n;
    return n;
}
hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_t *p, int) { memset(p, 0, sizeof(*p)); p->multiProcessorCount = 256; return hipSuccess; }
hipError_t hipMalloc(void **p, size_t n) { *p = malloc(n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void *p) { free(p); return hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t n, unsigned) { *p = malloc(n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipHostFree(void *p) { free(p); return hipSuccess; }
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) { memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemset(void *d, int v, size_t n) { memset(d, v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t) { memset(d, v, n); return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamQuery(hipStream_t) { return hipSuccess; }
// (device variables: the host-only build has their host shadows; no kernel runs here, so the shadow is the variable)
hipError_t hipMemcpyFromSymbol(void *d, const void *sym, size_t n, size_t off, hipMemcpyKind) { memcpy(d, (const char *)sym + off, n); return hipSuccess; }
hipError_t hipMemcpyToSymbol(const void *sym, const void *s, size_t n, size_t off, hipMemcpyKind) { memcpy((char *)const_cast<void *>(sym) + off, s, n); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { *s = (hipStream_t)malloc(8); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { free(s); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { *e = (hipEvent_t)malloc(8); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *e) { *e = (hipEvent_t)malloc(8); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { free(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0.0f; return hipSuccess; }
hipError_t hipFuncSetAttribute(const void *, hipFuncAttribute, int) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "hip_stub"; }
hipError_t hipLaunchKernel(const void *f, dim3, dim3, void **, size_t, hipStream_t)
{
    auto it = stub_names().find(f);
    stub_log().push_back(it == stub_names().end() ? std::string("?") : it->second);
    return hipSuccess;
}
hipError_t __hipPushCallConfiguration(dim3, dim3, size_t, hipStream_t) { return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3 *g, dim3 *b, size_t *s, hipStream_t *st) { *g = dim3(1); *b = dim3(1); *s = 0; *st = nullptr; return hipSuccess; }
void **__hipRegisterFatBinary(const void *) { static void *h; return &h; }
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *host_fn, char *, const char *name, unsigned, void *, void *, void *, void *, int *) { stub_names()[host_fn] = name; }
void __hipRegisterVar(void **, void *, char *, const char *, int, size_t, int, int) {}
}
