// beom_recorder.h — the one check every recorder of a handle passes before a call's first step: will it hold the records
// the call would write?  beom_step (the floats' track, the series, the tracer series) and beom_multi_step (the bands' series
// and tracer series) ask the same question in their own words.  Host only, no HIP header.
#pragma once
#include <cstddef>
#include <cstdio>

namespace beom_recorder {

// Can a recorder of nrec records, `held` of them taken, hold those due in steps tstp_first .. tstp_first+nsteps-1?  If not,
// the refusal goes to errm in the words of fmt (first step, last step, records due, stride, held, nrec).
inline bool holds(int tstp_first, int nsteps, int stride, size_t held, int nrec, char *errm, int errm_len, const char *fmt) {
    long long due = 0;
    for (int tstp = tstp_first; tstp < tstp_first + nsteps; ++tstp) due += tstp % stride == 0;
    if ((long long)held + due <= nrec) return true;
    if (errm && errm_len > 0) snprintf(errm, (size_t)errm_len, fmt, tstp_first, tstp_first + nsteps - 1, due, stride, (long long)held, nrec);
    return false;
}

}  // namespace beom_recorder
