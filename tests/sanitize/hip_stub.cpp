// hip_stub.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_sanitizers.py).  A stand-in for the HIP runtime so that the HOST code of
// libkws_mi355x.so -- the .kwsm parser, the plan builders, the table uploads, the argument checks of the C ABI -- can run under
// AddressSanitizer + UndefinedBehaviorSanitizer in a container without a GPU (SURVEY.md section 5 asked for a sanitizer run).
// "Device" memory is host heap (so an upload that reads past its source, or a plan table indexed out of range, is an ASan report),
// kernel launches do nothing and report success: NO arithmetic of the product runs here and nothing computes a result -- this is not
// a CPU path of the library, it is never linked into it, and nothing outside tests/ refers to it.
#include <hip/hip_runtime.h>

#include <cxxabi.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

// ---- recording (tests/test_fast_routes_host.py) ---------------------------------------------------------------------------
// KWS_STUB_RECORD=<file>: one line per device operation the host code enqueues -- kernel launches (the device name
// __hipRegisterFunction delivered for the host pointer, grid, block, dynamic LDS bytes, stream, the name demangled), memsets and copies (bytes; the target
// and a device source as "a<n>+<offset>": hipMalloc calls are numbered in order), event records and waits.  Streams and events are
// numbered by creation (0: the null stream).  kws_stub_note() puts a line of the driver's own into the file.  Unset: nothing is recorded.
namespace {
struct Rec {
    FILE *f = nullptr;
    std::map<const void *, std::string> kernel;                   // host pointer -> mangled device name
    std::map<const char *, std::pair<size_t, int>> alloc;         // live hipMalloc blocks: base -> (bytes, number)
    std::map<const void *, int> handle;                           // streams and events -> number
    int n_alloc = 0, n_handle = 0;
    dim3 grid{ 1 }, block{ 1 };
    size_t lds = 0;
    hipStream_t stream = nullptr;
};
Rec &rec()
{
    static Rec *r = nullptr;                                      // (kernels register from other units' constructors: built on first use)
    if (!r) {
        r = new Rec();
        const char *fn = getenv("KWS_STUB_RECORD");
        if (fn && *fn) r->f = fopen(fn, "w");
    }
    return *r;
}
std::string where(const void *p)
{
    Rec &r = rec();
    auto it = r.alloc.upper_bound((const char *)p);
    if (it != r.alloc.begin()) {
        --it;
        const size_t off = (size_t)((const char *)p - it->first);
        if (off < it->second.first) return "a" + std::to_string(it->second.second) + "+" + std::to_string(off);
    }
    return "host";
}
int number(const void *h) { if (!h) return 0; Rec &r = rec(); auto it = r.handle.find(h); return it == r.handle.end() ? -1 : it->second; }
void *new_handle() { void *h = malloc(8); Rec &r = rec(); r.handle[h] = ++r.n_handle; return h; }
void drop_handle(void *h) { rec().handle.erase(h); free(h); }
}  // namespace
#define REC(...) do { if (rec().f) { fprintf(rec().f, __VA_ARGS__); fflush(rec().f); } } while (0)

extern "C" {
void kws_stub_note(const char *line) { REC("%s\n", line); }
hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_t *p, int) { memset(p, 0, sizeof(*p)); p->multiProcessorCount = 256; return hipSuccess; }
hipError_t hipMalloc(void **p, size_t n)
{
    *p = malloc(n ? n : 1);
    if (!*p) return hipErrorOutOfMemory;
    Rec &r = rec();
    r.alloc[(const char *)*p] = { n ? n : 1, r.n_alloc++ };
    return hipSuccess;
}
hipError_t hipFree(void *p) { rec().alloc.erase((const char *)p); free(p); return hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t n, unsigned) { *p = malloc(n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipHostFree(void *p) { free(p); return hipSuccess; }
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind)
{
    REC("memcpy bytes=%zu dst=%s src=%s\n", n, where(d).c_str(), where(s).c_str());
    memcpy(d, s, n);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind, hipStream_t st)
{
    REC("memcpy_async bytes=%zu dst=%s src=%s stream=%d\n", n, where(d).c_str(), where(s).c_str(), number(st));
    memcpy(d, s, n);
    return hipSuccess;
}
hipError_t hipMemset(void *d, int v, size_t n)
{
    REC("memset bytes=%zu value=%d dst=%s\n", n, v, where(d).c_str());
    memset(d, v, n);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t st)
{
    REC("memset_async bytes=%zu value=%d dst=%s stream=%d\n", n, v, where(d).c_str(), number(st));
    memset(d, v, n);
    return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamQuery(hipStream_t) { return hipSuccess; }
// (device variables: the host-only build has their host shadows; no kernel runs here, so the shadow is the variable)
hipError_t hipMemcpyFromSymbol(void *d, const void *sym, size_t n, size_t off, hipMemcpyKind) { memcpy(d, (const char *)sym + off, n); return hipSuccess; }
hipError_t hipMemcpyToSymbol(const void *sym, const void *s, size_t n, size_t off, hipMemcpyKind) { memcpy((char *)const_cast<void *>(sym) + off, s, n); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { *s = (hipStream_t)new_handle(); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { drop_handle(s); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { REC("stream_wait event=%d stream=%d\n", number(e), number(s)); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { *e = (hipEvent_t)new_handle(); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *e) { *e = (hipEvent_t)new_handle(); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { drop_handle(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { REC("event_record event=%d stream=%d\n", number(e), number(s)); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0.0f; return hipSuccess; }
hipError_t hipFuncSetAttribute(const void *, hipFuncAttribute, int) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "hip_stub"; }
hipError_t hipLaunchKernel(const void *fn, dim3 g, dim3 b, void **, size_t lds, hipStream_t st)
{
    if (rec().f) {
        auto it = rec().kernel.find(fn);
        const char *name = it == rec().kernel.end() ? "?" : it->second.c_str();
        char *plain = abi::__cxa_demangle(name, nullptr, nullptr, nullptr);
        REC("launch %s grid=%u,%u,%u block=%u,%u,%u lds=%zu stream=%d | %s\n", name, g.x, g.y, g.z, b.x, b.y, b.z, lds, number(st), plain ? plain : name);
        free(plain);
    }
    return hipSuccess;
}
// (a <<< >>> launch pushes its configuration, the kernel's host stub pops it and calls hipLaunchKernel with it)
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t s, hipStream_t st) { Rec &r = rec(); r.grid = g; r.block = b; r.lds = s; r.stream = st; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3 *g, dim3 *b, size_t *s, hipStream_t *st) { Rec &r = rec(); *g = r.grid; *b = r.block; *s = r.lds; *st = r.stream; return hipSuccess; }
void **__hipRegisterFatBinary(const void *) { static void *h; return &h; }
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *host_fn, char *, const char *device_name, unsigned, void *, void *, void *, void *, int *) { rec().kernel[host_fn] = device_name; }
void __hipRegisterVar(void **, void *, char *, const char *, int, size_t, int, int) {}
}
