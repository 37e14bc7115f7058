// comm_rccl.cpp -- zk_comm over RCCL (xGMI within a node): one process per GPU.  The collectives run on the stream
// shard.hip hands in (the prover's exchange stream, ordered after its compute stream by an event), so they overlap
// the compute that does not wait for them.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <string>

#include "../../include/zkvm_gpu.h"
#include "comm.hpp"
#include "prover_internal.hpp"

namespace {

struct RcclComm : zk_comm {
    ncclComm_t comm = nullptr;
    // the control channel's staging (control_gather): CTL_CAP bytes to send, then world x CTL_CAP received
    static constexpr size_t CTL_CAP = 2048;
    int device = 0;
    uint8_t *ctl = nullptr;
    hipStream_t ctl_st = nullptr;
    ~RcclComm() override {
        if (comm) ncclCommDestroy(comm);
        if (ctl) (void)hipFree(ctl);
        if (ctl_st) (void)hipStreamDestroy(ctl_st);
    }
    bool loopback() const override { return false; }
    int all_to_all(const std::vector<zk_prover *> &P, const std::vector<const void *> &send,
                   const std::vector<void *> &recv, size_t bytes, hipStream_t is) override {
        if (P.size() != 1) ZK_FAIL(ZK_ERR_INVALID_ARG, "an RCCL communicator drives exactly one local rank");
        ncclResult_t r = ncclAllToAll(send[0], recv[0], bytes, ncclUint8, comm, is);
        if (r != ncclSuccess) ZK_FAIL(ZK_ERR_DEVICE, std::string("ncclAllToAll: ") + ncclGetErrorString(r));
        return ZK_OK;
    }
    int all_gather(const std::vector<zk_prover *> &P, const std::vector<const void *> &send,
                   const std::vector<void *> &recv, size_t bytes, hipStream_t is) override {
        if (P.size() != 1) ZK_FAIL(ZK_ERR_INVALID_ARG, "an RCCL communicator drives exactly one local rank");
        ncclResult_t r = ncclAllGather(send[0], recv[0], bytes, ncclUint8, comm, is);
        if (r != ncclSuccess) ZK_FAIL(ZK_ERR_DEVICE, std::string("ncclAllGather: ") + ncclGetErrorString(r));
        return ZK_OK;
    }
    // (compiled, never run: no machine with two GPUs has built this project -- DESIGN.md section 7)
    int control_gather(const void *send, void *recv, size_t bytes) override {
        if (bytes > CTL_CAP) ZK_FAIL(ZK_ERR_INVALID_ARG, "control exchange larger than the communicator's staging");
        ZK_CHECK_HIP(hipSetDevice(device));
        ZK_CHECK_HIP(hipMemcpyAsync(ctl, send, bytes, hipMemcpyHostToDevice, ctl_st));
        ncclResult_t r = ncclAllGather(ctl, ctl + CTL_CAP, bytes, ncclUint8, comm, ctl_st);
        if (r != ncclSuccess) ZK_FAIL(ZK_ERR_DEVICE, std::string("ncclAllGather (control): ") + ncclGetErrorString(r));
        ZK_CHECK_HIP(hipMemcpyAsync(recv, ctl + CTL_CAP, bytes * (size_t)world, hipMemcpyDeviceToHost, ctl_st));
        ZK_CHECK_HIP(hipStreamSynchronize(ctl_st));
        return ZK_OK;
    }
};

}  // namespace

int zk_rccl_unique_id(unsigned char id[128]) {
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    ncclUniqueId u;
    ncclResult_t r = ncclGetUniqueId(&u);
    if (r != ncclSuccess) ZK_FAIL(ZK_ERR_DEVICE, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
    memcpy(id, &u, 128);
    return ZK_OK;
}

int zk_make_rccl_comm(const unsigned char id[128], int rank, int world, int device, zk_comm **out) {
    ZK_CHECK_HIP(hipSetDevice(device));
    ncclUniqueId u;
    memcpy(&u, id, 128);
    auto *c = new RcclComm();
    c->world = world;
    c->rank = rank;
    c->device = device;
    if (hipMalloc(&c->ctl, RcclComm::CTL_CAP * (size_t)(world + 1)) != hipSuccess ||
        hipStreamCreateWithFlags(&c->ctl_st, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        ZK_FAIL(ZK_ERR_OUT_OF_MEMORY, "the control channel's staging buffer could not be allocated");
    }
    ncclResult_t r = ncclCommInitRank(&c->comm, world, u, rank);
    if (r != ncclSuccess) {
        delete c;
        ZK_FAIL(ZK_ERR_DEVICE, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
    }
    *out = c;
    return ZK_OK;
}
