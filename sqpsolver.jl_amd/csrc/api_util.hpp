// api_util.hpp -- what the two files of the extern "C" boundary share (api.hip: create / destroy, the seat, merit, the SQP run
// and the shared queue calls; api_models.hip: the attach, set-instance and value-queue calls).
#pragma once
#include "ctx.hpp"
#include <string>

namespace sqphip {

template <class F> int guarded(sqphip_ctx *h, F &&f)
{
    try {
        SQPHIP_HIP_OK(hipSetDevice(h->c.opt.device));
        return f(h->c);
    } catch (const std::string &e) {
        h->c.err = e;
        return SQPHIP_EHIP;
    } catch (const std::bad_alloc &) {
        h->c.err = "out of host memory";
        return SQPHIP_ENOMEM;
    }
}

inline void h2d(Ctx &C, double *dst, const double *src, size_t k)
{
    if (src && k) SQPHIP_HIP_OK(hipMemcpyAsync(dst, src, sizeof(double) * k, hipMemcpyHostToDevice, C.stream));
}
inline void d2h(Ctx &C, double *dst, const double *src, size_t k)
{
    if (dst && k) SQPHIP_HIP_OK(hipMemcpyAsync(dst, src, sizeof(double) * k, hipMemcpyDeviceToHost, C.stream));
}

// (re)build the lanes from the owner's current device view (api.hip; after sqphip_create and after every *_attach)
void make_lanes(Ctx &C);
// the tables of a scenario queue (api_models.hip); nv: doubles of a scenario's block of values, < 0: the ACOPF tables
int stream_begin(sqphip_ctx *h, int32_t n_scenarios, int32_t keep_multipliers, long nv);

// The tables of sqphip_acopf_set_* and of the ACOPF scenario queue (sqphip_sqp_stream_begin / _set) exist on a context
// attached with one of the three ACOPF forms only: on a dense, QCQP or factorable-NLP context those entry points are
// refused here, on the host, before anything touches the device.  Returns 0 on an ACOPF (or unattached) context.
inline int acopf_only(sqphip_ctx *h, const char *fn)
{
    if (!h) return 0;
    const DV &d = h->c.d;
    const char *what = d.qc ? "a QCQP context (sqphip_qcqp_attach; use sqphip_qcqp_set_instance, sqphip_qcqp_stream_begin / _set)"
                     : d.nlp ? "an NLP context (sqphip_nlp_attach; use sqphip_nlp_set_instance, sqphip_nlp_stream_begin / _set)"
                     : d.dense_nlp ? "a dense context (sqphip_dense_attach; use sqphip_dense_set_instance)" : nullptr;
    if (!what) return 0;
    h->c.err = std::string(fn) + ": not available on " + what;
    return SQPHIP_EINVAL;
}

}  // namespace sqphip
