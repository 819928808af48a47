// The RCCL communicator of one-process-per-GPU runs and the gathers of a
// plan's phases and statistics to one rank (C-ABI in include/slm_hip.h).
#include <rccl/rccl.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "plan.hpp"

using namespace slm;

namespace {

ncclComm_t g_comm = nullptr;
int g_comm_rank = 0, g_comm_size = 1;

// Root side of a gather on stream `st`: grow the destination slab to `elems`
// elements, then one grouped receive per peer (one xGMI hop each) and the
// root's own slab, `local`, as a device copy.
int receive_slabs(GatherState::Slab& dst_slab, const std::vector<long long>& off, size_t elem, ncclDataType_t dt,
                  int me, const void* local, hipStream_t st) {
    const int n = (int)off.size() - 1;
    const long long elems = off[n];
    if (dst_slab.elems < elems) {
        HIP_TRY(hipStreamSynchronize(st));  // earlier gathers into the old buffer
        if (dst_slab.buf) HIP_TRY(hipFree(dst_slab.buf));
        dst_slab.buf = nullptr;
        dst_slab.elems = 0;
        HIP_TRY(hipMalloc(&dst_slab.buf, std::max<long long>(elems, 1) * elem));
        dst_slab.elems = elems;
    }
    char* dst = static_cast<char*>(dst_slab.buf);
    if (n > 1) NCCL_TRY(ncclGroupStart());
    for (int r = 0; r < n; ++r) {
        const size_t cnt = (size_t)(off[r + 1] - off[r]);
        if (!cnt) continue;
        if (r == me)
            HIP_TRY(hipMemcpyAsync(dst + off[r] * elem, local, cnt * elem, hipMemcpyDeviceToDevice, st));
        else
            NCCL_TRY(ncclRecv(dst + off[r] * elem, cnt, dt, r, g_comm, st));
    }
    if (n > 1) NCCL_TRY(ncclGroupEnd());
    return 0;
}

// Gather one per-hologram slab of every rank to `root` (rank order): `src`
// holds this rank's counts[me] x per_item elements of `elem` bytes (RCCL type
// `dt`); on root the concatenation lands in `dst` (grown as needed) and, if
// host_out, on the host. Default: grouped ncclSend / ncclRecv and the root's
// own slab as a device copy, on the plan stream.
// Staged ($SLM_GATHER_STAGED=1): the slab is first copied into one of two
// staging buffers on the plan stream (so the next run, queued behind that
// copy, may overwrite `src`), then the comm stream -- behind an event -- moves
// it, overlapping the next run. Stream-ordered either way, no host
// synchronisation unless host_out.
int gather_slab(slm_plan* p, const void* src, long long per_item, size_t elem, ncclDataType_t dt, const int* counts,
                int root, GatherState::Slab& dst, void* host_out) {
    if (!p || !counts) return fail(SLM_ERR_ARG, "null argument");
    Engine* e = nullptr;
    RC(engine_of(p, &e));
    PlanState& s = p->s;
    GatherState& g = p->gather;
    HIP_TRY(hipSetDevice(s.device));
    const int n = g_comm ? g_comm_size : 1;
    const int me = g_comm ? g_comm_rank : 0;
    if (root < 0 || root >= n) return fail(SLM_ERR_ARG, "root %d outside [0, %d)", root, n);
    if (counts[me] != s.B) return fail(SLM_ERR_ARG, "counts[%d]=%d but the plan holds %d", me, counts[me], s.B);
    // a GD run on the one-launch column side may have faulted (its grid wait gave
    // up): settle it -- redo it on two launches -- before its results leave this
    // rank. Only a fused run queued since the last check can have (no host sync
    // per gather otherwise)
    if (e->unsettled()) RC(slm_plan_sync(p));
    std::vector<long long> off(n + 1);
    RC(slm_gather_layout(n, counts, per_item, off.data()));
    if (me != root && !g_comm) return fail(SLM_ERR_COMM, "no communicator");
    // $SLM_GATHER_STAGED=1: stage the slab and move it on the plan's comm stream
    // (overlaps the next run). Off by default: at 1024^2 the second stream cost
    // 0.28 ms per 200-iteration run on one GPU (272-275 against 295-296
    // holograms/s, profiles/r05/gather_ab_s7.txt), more than rank 0's wait for
    // seven 4 MB receives is expected to cost. Read per call (tests switch it).
    const char* st_env = std::getenv("SLM_GATHER_STAGED");
    const bool staged = st_env && std::atoi(st_env) != 0;
    hipStream_t st = s.stream;  // the stream that moves the slab
    const void* local = src;    // what it moves
    int k = -1;                 // staging slot
    if (!staged) {
        // a staged gather still queued on the comm stream may write the same buffer
        RC(gather_order_after(g, s.stream));
        g.last = -1;
    } else {
        if (!g.comm_stream) {
            HIP_TRY(hipStreamCreateWithFlags(&g.comm_stream, hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&g.ready, hipEventDisableTiming));
            for (int i = 0; i < 2; ++i) HIP_TRY(hipEventCreateWithFlags(&g.done[i], hipEventDisableTiming));
        }
        const size_t mine = (size_t)(off[me + 1] - off[me]) * elem;
        k = g.stage_next;
        g.stage_next ^= 1;
        if (g.stage_cap[k] < mine) {
            HIP_TRY(hipStreamSynchronize(g.comm_stream));  // nothing may still read the old buffer
            if (g.stage[k]) HIP_TRY(hipFree(g.stage[k]));
            g.stage[k] = nullptr;
            g.stage_cap[k] = 0;
            HIP_TRY(hipMalloc(&g.stage[k], mine));
            g.stage_cap[k] = mine;
        }
        // plan stream: wait for the send that last read this staging buffer, copy the slab
        if (g.done_set[k]) HIP_TRY(hipStreamWaitEvent(s.stream, g.done[k], 0));
        if (mine) HIP_TRY(hipMemcpyAsync(g.stage[k], src, mine, hipMemcpyDeviceToDevice, s.stream));
        HIP_TRY(hipEventRecord(g.ready, s.stream));
        st = g.comm_stream;
        local = g.stage[k];
        HIP_TRY(hipStreamWaitEvent(st, g.ready, 0));
    }
    if (me == root)
        RC(receive_slabs(dst, off, elem, dt, me, local, st));
    else if (s.B)
        NCCL_TRY(ncclSend(local, (size_t)s.B * per_item, dt, root, g_comm, st));
    if (staged) {
        HIP_TRY(hipEventRecord(g.done[k], st));
        g.done_set[k] = true;
        g.last = k;
    }
    // a device-side gather stays stream-ordered (slm_plan_sync, a read or the
    // stopwatch wait for it); a host copy waits here
    if (me == root && host_out && off[n]) {
        HIP_TRY(hipStreamSynchronize(st));
        RC(copy_sync(host_out, dst.buf, (size_t)off[n] * elem, hipMemcpyDeviceToHost, st));
    }
    return 0;
}

}  // namespace

namespace slm {

int gather_order_after(GatherState& g, hipStream_t stream) {
    if (g.last >= 0) HIP_TRY(hipStreamWaitEvent(stream, g.done[g.last], 0));
    return 0;
}

void gather_free(GatherState& g) {
    if (g.comm_stream) (void)hipStreamSynchronize(g.comm_stream);  // gathers still reading / writing
    for (void* ptr : {g.phase.buf, g.stats.buf, g.stop.buf, g.stage[0], g.stage[1]})
        if (ptr) (void)hipFree(ptr);
    for (hipEvent_t e : {g.done[0], g.done[1], g.ready})
        if (e) (void)hipEventDestroy(e);
    if (g.comm_stream) (void)hipStreamDestroy(g.comm_stream);
    g = GatherState();
}

}  // namespace slm

extern "C" {

int slm_comm_unique_id(unsigned char* id128) {
    if (!id128) return fail(SLM_ERR_ARG, "null argument");
    ncclUniqueId id;
    NCCL_TRY(ncclGetUniqueId(&id));
    std::memcpy(id128, id.internal, NCCL_UNIQUE_ID_BYTES);
    return 0;
}

int slm_comm_init(int nranks, int rank, const unsigned char* id128) {
    if (!id128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(SLM_ERR_ARG, "bad communicator arguments");
    RC(ensure_device());
    if (g_comm) {
        ncclCommDestroy(g_comm);
        g_comm = nullptr;
    }
    ncclUniqueId id;
    std::memcpy(id.internal, id128, NCCL_UNIQUE_ID_BYTES);
    NCCL_TRY(ncclCommInitRank(&g_comm, nranks, id, rank));
    g_comm_rank = rank;
    g_comm_size = nranks;
    return 0;
}

int slm_comm_destroy(void) {
    if (g_comm) {
        // device gathers return without waiting: let queued RCCL work finish first
        (void)hipDeviceSynchronize();
        ncclCommDestroy(g_comm);
        g_comm = nullptr;
    }
    return 0;
}

int slm_gather_layout(int nranks, const int* counts, long long per_item, long long* offsets) {
    if (nranks < 1 || !counts || !offsets || per_item < 0) return fail(SLM_ERR_ARG, "bad gather layout arguments");
    long long off = 0;
    for (int r = 0; r < nranks; ++r) {
        if (counts[r] < 0) return fail(SLM_ERR_ARG, "counts[%d] = %d is negative", r, counts[r]);
        offsets[r] = off;
        off += (long long)counts[r] * per_item;
    }
    offsets[nranks] = off;
    return 0;
}

int slm_plan_gather_phase(slm_plan* p, const int* counts, int root, float* host_out) {
    if (!p) return fail(SLM_ERR_ARG, "null plan");
    return gather_slab(p, p->s.phase_out, p->s.holo, sizeof(float), ncclFloat32, counts, root, p->gather.phase,
                       host_out);
}

int slm_plan_time_gather(slm_plan* p, const int* counts, int root, int reps, double* ms, long long* bytes_out) {
    if (!p || !counts || !ms || reps < 1) return fail(SLM_ERR_ARG, "bad gather-timing arguments");
    RC(slm_plan_sync(p));
    const int me = g_comm ? g_comm_rank : 0;
    hipStream_t st = p->s.stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    int rc = 0;
    float t = 0.f;
    if (hipEventRecord(e0, st) != hipSuccess) rc = fail(SLM_ERR_HIP, "event record failed");
    for (int i = 0; i < reps && !rc; ++i) rc = slm_plan_gather_phase(p, counts, root, nullptr);
    // the transfers run on the comm stream: the stop event follows the last one
    if (!rc && p->gather.last >= 0 && hipStreamWaitEvent(st, p->gather.done[p->gather.last], 0) != hipSuccess)
        rc = fail(SLM_ERR_HIP, "gather timing wait failed");
    if (!rc && (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                hipEventElapsedTime(&t, e0, e1) != hipSuccess))
        rc = fail(SLM_ERR_HIP, "gather timing events failed");
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc;
    *ms = (double)t / reps;
    if (bytes_out) *bytes_out = me == root ? 0 : (long long)p->s.B * p->s.holo * (long long)sizeof(float);
    return 0;
}

int slm_plan_gather_stats(slm_plan* p, const int* counts, int root, double* stats_out, int* iters_out) {
    if (!p) return fail(SLM_ERR_ARG, "null plan");
    // per hologram: [max_loops][4] doubles (max E, sum E^2, sum E T, error), then the stop index
    RC(gather_slab(p, p->s.stats, (long long)p->s.max_loops * 4, sizeof(double), ncclFloat64, counts, root,
                   p->gather.stats, stats_out));
    RC(gather_slab(p, p->s.stop, 1, sizeof(int), ncclInt32, counts, root, p->gather.stop, iters_out));
    if (iters_out && (g_comm ? g_comm_rank : 0) == root) {  // as slm_plan_read reports it
        long long total = 0;
        for (int r = 0; r < (g_comm ? g_comm_size : 1); ++r) total += counts[r];
        stop_to_iterations(iters_out, total);
    }
    return 0;
}

}  // extern "C"
