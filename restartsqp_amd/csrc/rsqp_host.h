// rsqp_host.h -- what every host translation unit of the C ABI shares: how an entry point reports an error, the status mapping, and
// the accessors through which rsqp_rccl.cpp reaches a batch (struct rsqp_batch is private to the batch units: rsqp_batch.h).
#pragma once
#include <string>

#include "../../include/rsqp_hip.h"
#include "rsqp_internal.h"

int rsqp_fail_msg(int code, const char *msg);   // rsqp_api.hip: sets rsqp_last_error() of the calling thread, returns code
inline int fail(int code, const std::string &msg) { return rsqp_fail_msg(code, msg.c_str()); }
#define HIPCHK(call)                                                                                              \
    do {                                                                                                          \
        hipError_t e_ = (call);                                                                                   \
        if (e_ != hipSuccess)                                                                                     \
            return rsqp_fail_msg(RSQP_ERR_DEVICE, (std::string(#call) + ": " + hipGetErrorString(e_)).c_str());   \
    } while (0)

struct SmallPlan;                               // rsqp_small_plan.h
void rsqp_plan_words(const SmallPlan &pl, int *out);   // rsqp_api.hip: the plan as the RSQP_PLAN_OUT_WORDS words of rsqp_hip.h

inline int exitflag_of(int status_word, int ret) {
    // qpOASESInterface::get_status (src/qpOASESInterface.cpp:332-357)
    if (status_word >= 200) return RSQP_QPERROR_UNBOUNDED;
    if (status_word >= 100) return RSQP_QPERROR_INFEASIBLE;
    if (status_word == QPS_SOLVED) return RSQP_QP_OPTIMAL;
    (void)ret;
    switch (status_word) {
    case QPS_NOTINITIALISED: return RSQP_QPERROR_NOTINITIALISED;
    case QPS_PREPARINGAUXILIARYQP: return RSQP_QPERROR_PREPARINGAUXILIARYQP;
    case QPS_AUXILIARYQPSOLVED: return RSQP_QPERROR_AUXILIARYQPSOLVED;
    case QPS_PERFORMINGHOMOTOPY: return RSQP_QPERROR_PERFORMINGHOMOTOPY;
    case QPS_HOMOTOPYQPSOLVED: return RSQP_QPERROR_HOMOTOPYQPSOLVED;
    }
    return RSQP_QPERROR_UNKNOWN;
}

// rsqp_batch.hip: the native RCCL call sites (rsqp_rccl.cpp) reach the batch through these
hipStream_t rsqp_batch_stream_internal(rsqp_batch *b);
int rsqp_batch_device_internal(const rsqp_batch *b);
int rsqp_batch_nq_internal(const rsqp_batch *b);
