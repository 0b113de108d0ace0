// ssf_exchange.hpp -- RCCL as the library resolves it at run time, and what of ssf_exchange.hip the frame path of ssf_host.hip calls
// itself.  Private to those two files: <rccl/rccl.h> stays out of ssf_handle.hpp, which only holds communicators.
#pragma once
#include <rccl/rccl.h>          // types only: the library is resolved at run time (dlopen), never linked
#include "ssf_handle.hpp"

#pragma GCC visibility push(hidden)
struct RcclApi {
    void* lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;
    decltype(&ncclCommUserRank) CommUserRank = nullptr;
    decltype(&ncclBroadcast) Broadcast = nullptr;           // the three below: only the dealt extract stage needs them (ssf_comm_deal_extract)
    decltype(&ncclCommSplit) CommSplit = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    std::string err;
};
RcclApi* rccl_api();                          // nullptr: no RCCL in this process
int comm_gather_counts(ssf_handle* h);
int comm_counts(ssf_handle* h);
#pragma GCC visibility pop

#define NCK(call)                                                                                    \
    do {                                                                                             \
        ncclResult_t r_ = (call);                                                                    \
        if (r_ != ncclSuccess) {                                                                     \
            RcclApi* a_ = rccl_api();                                                                \
            h->err = std::string(#call) + ": " + ((a_ && a_->GetErrorString) ? a_->GetErrorString(r_) : "RCCL error"); \
            return SSF_ERR_DEVICE;                                                                   \
        }                                                                                            \
    } while (0)
