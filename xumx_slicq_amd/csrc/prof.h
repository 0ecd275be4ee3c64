// Optional per-kernel timing with HIP events recorded on the launch stream
// (bench.py reads it for the roofline object; off by default, zero cost when off).
#pragma once
#include "common.h"

namespace xsq {
bool prof_enabled();
bool prof_wanted(const char* name);
void prof_begin(const char* name, hipStream_t stream, const char* name2 = nullptr);
void prof_end(hipStream_t stream);

struct ProfScope {
    hipStream_t s;
    bool on;
    ProfScope(const char* name, hipStream_t stream) : s(stream), on(prof_wanted(name)) {
        if (on) prof_begin(name, s);
    }
    // one launch that does the work of two event names: one event pair, half of its time and one launch under each
    ProfScope(const char* name, const char* name2, hipStream_t stream) : s(stream), on(prof_wanted(name) || prof_wanted(name2)) {
        if (on) prof_begin(name, s, name2);
    }
    ~ProfScope() {
        if (on) prof_end(s);
    }
};
}  // namespace xsq

#define XSQ_PROF(name, stream) ::xsq::ProfScope prof_scope_##__LINE__(name, stream)
