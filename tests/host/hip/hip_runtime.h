// A stand-in for <hip/hip_runtime.h>, for compiling xfr_amd/csrc/hip_owner.h with the host compiler alone (hip_owner_check.cpp): the types and the
// create / destroy calls that header uses, backed by malloc, with a live-object counter per kind, a log of the calls, and a switch that makes the
// k-th creation from now fail.
#pragma once
#include <cstdlib>
#include <string>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorUnknown = 999 };
typedef struct fake_event* hipEvent_t;
typedef struct fake_stream* hipStream_t;
enum { hipEventDefault = 0, hipEventDisableTiming = 2, hipStreamNonBlocking = 1, hipHostMallocDefault = 0 };

namespace fake {
enum Kind { DEVICE, PINNED, EVENT, STREAM, KINDS };
inline int live[KINDS];
inline std::string calls;                  // one letter per call: m/f device, h/u pinned, e/d event, s/x stream, Y device synchronise
inline int fail_in = 0;                    // > 0: the fail_in-th creation from now fails with fail_with
inline hipError_t fail_with = hipErrorOutOfMemory;
inline hipError_t create(Kind k, char letter, void** out)
{
    calls += letter;
    if (fail_in > 0 && --fail_in == 0) return fail_with;
    *out = malloc(16);
    ++live[k];
    return hipSuccess;
}
inline hipError_t destroy(Kind k, char letter, void* p)
{
    calls += letter;
    free(p);
    --live[k];
    return hipSuccess;
}
}  // namespace fake

inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : "unknown error"; }
inline hipError_t hipMalloc(void** p, size_t) { return fake::create(fake::DEVICE, 'm', p); }
inline hipError_t hipFree(void* p) { return fake::destroy(fake::DEVICE, 'f', p); }
inline hipError_t hipHostMalloc(void** p, size_t, unsigned) { return fake::create(fake::PINNED, 'h', p); }
inline hipError_t hipHostFree(void* p) { return fake::destroy(fake::PINNED, 'u', p); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return fake::create(fake::EVENT, 'e', (void**)e); }
inline hipError_t hipEventDestroy(hipEvent_t e) { return fake::destroy(fake::EVENT, 'd', e); }
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return fake::create(fake::STREAM, 's', (void**)s); }
inline hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { return fake::create(fake::STREAM, 's', (void**)s); }
inline hipError_t hipStreamDestroy(hipStream_t s) { return fake::destroy(fake::STREAM, 'x', s); }
inline hipError_t hipDeviceSynchronize() { fake::calls += 'Y'; return hipSuccess; }
