// bicg_exchange.hip -- the small kernels between the products and the element-wise phases: the scalar recurrences applied on
// their own (k_apply, k_apply_p2p), the halo pack / push / unpack kernels and the peer-to-peer transport's barrier and self-tests.
#include "bicg_device.h"
#include "bicg_devfn.h"
#include "bicg_reduce.h"
#include "bicg_knobs.h"
#include "bicg_launch.h"

namespace bicg {

__global__ void __launch_bounds__(kBlock) k_apply(Scal *S, int phase)
{
    if (S->done) return;
    apply_phase_block<true>(S, phase);
}

__global__ void __launch_bounds__(kBlock) k_apply_p2p(Scal *S, int phase, int n, P2pRed pr, unsigned long long timeout_ticks)
{
    if (S->done) return;
    __shared__ double vals[kRedSlots * kMaxRanksP2p];
    __shared__ int s_fail;
    if (!p2p_collect(S, n, pr, timeout_ticks, vals, &s_fail)) return;
    if (phase != PH_NONE) apply_phase_block<true>(S, phase);
}

__global__ void __launch_bounds__(kBlock) k_p2p_selftest(P2pRed pr, unsigned seq0, int rounds, unsigned long long timeout_ticks,
                                                         int *status)
{
    __shared__ double vals[kRedSlots * kMaxRanksP2p];
    __shared__ double expect[kRedSlots * kMaxRanksP2p];
    __shared__ int s_timeout;
    constexpr int n = kMaxDots;
    if (threadIdx.x == 0) s_timeout = 0;
    __syncthreads();
    for (int r = 0; r < rounds; ++r) {
        const unsigned seq = seq0 + (unsigned)r;
        for (int t = threadIdx.x; t < n * pr.nranks; t += kBlock) {
            const int p = t / n, d = t % n;
            ll_store(pr.mail[p] + mail_index(seq, pr.nranks, pr.rank, d), selftest_value(pr.rank, seq, d), seq);
        }
        for (int t = threadIdx.x; t < n * pr.nranks; t += kBlock) {
            const int p = t / n, d = t % n;
            double v;
            if (!ll_wait(pr.mail[pr.rank] + mail_index(seq, pr.nranks, p, d), seq, timeout_ticks, &v)) s_timeout = 1;
            vals[p * kRedSlots + d] = v;
            expect[p * kRedSlots + d] = selftest_value(p, seq, d);
        }
        __syncthreads();
        if (s_timeout) {                 // a peer is not answering: do not wait `rounds` time-outs
            if (threadIdx.x == 0) atomicAdd(&status[1], 1);
            return;
        }
        if ((int)threadIdx.x < n) {
            const double got = rank_tree_sum(vals + threadIdx.x, pr.nranks);
            const double want = rank_tree_sum(expect + threadIdx.x, pr.nranks);
            if (!(got == want)) atomicAdd(&status[0], 1);
        }
        __syncthreads();
    }
}

void launch_apply(Scal *S, int phase, hipStream_t st)
{
    BICG_LAUNCH(k_apply, dim3(1), dim3(phase >= PH_SH_INIT ? kBlock : 1), 0, st, S, phase);
}

// gather the entries of x other ranks need into the contiguous send buffer
__global__ void __launch_bounds__(kBlock) k_halo_pack(const double *x, const uint32_t *idx, uint32_t n, double *out, const Scal *S)
{
    if (S->done) return;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) out[i] = x[idx[i]];
}

void launch_halo_pack(const double *x, const uint32_t *send_idx, uint32_t nsend, double *sendbuf, Scal *S, hipStream_t st)
{
    if (nsend == 0) return;
    unsigned g = (nsend + kBlock - 1) / kBlock;
    if (g > 1024) g = 1024;
    BICG_LAUNCH(k_halo_pack, dim3(g), dim3(kBlock), 0, st, x, send_idx, nsend, sendbuf, S);
}

// The same for the nvec vectors of a set (blockIdx.y: the vector), into ONE send buffer laid out peer-major: what goes to peer p
// is one contiguous block (nvec * scnt[p] doubles from nvec * sdsp[p]) with vector j at + j * scnt[p], so a single transport
// exchange with counts and displacements scaled by nvec carries the set. map[i] = {sdsp[p], scnt[p]} of entry i's peer.
__global__ void __launch_bounds__(kBlock) k_halo_pack_set(const double *x, size_t stride, const uint32_t *idx, const uint2 *map, uint32_t n,
                                                          double *out, const Scal *S)
{
    if (S->done) return;
    const uint32_t j = blockIdx.y, nvec = gridDim.y;
    const double *xj = x + (size_t)j * stride;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const uint2 m = map[i];
        out[(size_t)nvec * m.x + (size_t)j * m.y + (i - m.x)] = xj[idx[i]];
    }
}

void launch_halo_pack_set(const double *x, size_t stride, int nvec, const uint32_t *send_idx, const uint2 *map, uint32_t nsend, double *sendbuf,
                          const Scal *S, hipStream_t st)
{
    if (nsend == 0 || nvec < 1) return;
    unsigned g = (nsend + kBlock - 1) / kBlock;
    if (g > 1024) g = 1024;
    BICG_LAUNCH(k_halo_pack_set, dim3(g, (unsigned)nvec), dim3(kBlock), 0, st, x, stride, send_idx, map, nsend, sendbuf, S);
}

// ... and the landing buffer (same layout, map[i] = {rdsp[p], rcnt[p]} of halo entry i's owner) scattered into the halo tails of
// the vectors: tail + j * stride + i, i < halo -- inside vector j's own stride, the slack behind the last vector stays untouched
__global__ void __launch_bounds__(kBlock) k_halo_unpack_set(const double *in, const uint2 *map, uint32_t n, double *tail, size_t stride,
                                                            const Scal *S)
{
    if (S->done) return;
    const uint32_t j = blockIdx.y, nvec = gridDim.y;
    double *tj = tail + (size_t)j * stride;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const uint2 m = map[i];
        tj[i] = in[(size_t)nvec * m.x + (size_t)j * m.y + (i - m.x)];
    }
}

void launch_halo_unpack_set(const double *recvbuf, const uint2 *map, uint32_t halo, int nvec, double *tail, size_t stride, const Scal *S,
                            hipStream_t st)
{
    if (halo == 0 || nvec < 1) return;
    unsigned g = (halo + kBlock - 1) / kBlock;
    if (g > 1024) g = 1024;
    BICG_LAUNCH(k_halo_unpack_set, dim3(g, (unsigned)nvec), dim3(kBlock), 0, st, recvbuf, map, halo, tail, stride, S);
}

void launch_apply_p2p(Scal *S, int phase, int n, const P2pRed &pr, unsigned long long timeout_ticks, hipStream_t st)
{
    BICG_LAUNCH(k_apply_p2p, dim3(1), dim3(kBlock), 0, st, S, phase, n, pr, timeout_ticks);
}

__global__ void __launch_bounds__(kBlock) k_halo_push(const double *x, const uint32_t *idx, uint32_t n,
                                                      const unsigned long long *dst0, const unsigned long long *dst_stride,
                                                      unsigned seq, const Scal *S)
{
    if (S->done) return;
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    llword *dst = reinterpret_cast<llword *>(dst0[i] + (unsigned long long)(seq % kHaloRing) * dst_stride[i]);
    ll_store(dst, x[idx[i]], seq);
}

void launch_halo_push(const double *x, const uint32_t *send_idx, uint32_t nsend, const unsigned long long *dst0,
                      const unsigned long long *dst_stride, unsigned seq, Scal *S, hipStream_t st)
{
    if (nsend == 0) return;
    BICG_LAUNCH(k_halo_push, dim3((nsend + kBlock - 1) / kBlock), dim3(kBlock), 0, st, x, send_idx, nsend, dst0,
                       dst_stride, seq, (const Scal *)S);
}

__global__ void __launch_bounds__(kBlock) k_halo_unpack(const llword *ring, uint32_t halo, unsigned seq, double *tail, Scal *S,
                                                        unsigned long long timeout_ticks)
{
    if (S->done) return;
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= halo) return;
    double v;
    if (ll_wait(ring + ((size_t)(seq % kHaloRing) * halo + i) * 2, seq, timeout_ticks, &v)) {
        tail[i] = v;
    } else {
        S->comm_error = 1;
        S->done = 1;
    }
}

void launch_halo_unpack(const llword *ring, uint32_t halo, unsigned seq, double *tail, Scal *S,
                        unsigned long long timeout_ticks, hipStream_t st)
{
    if (halo == 0) return;
    BICG_LAUNCH(k_halo_unpack, dim3((halo + kBlock - 1) / kBlock), dim3(kBlock), 0, st, ring, halo, seq, tail, S,
                       timeout_ticks);
}

// Flow control for halo exchanges that are not separated by an all-reduce: every rank posts a token
// to every rank (slot kRedSlots-1 of the mailbox, its own sequence numbers) and waits for all P.
__global__ void __launch_bounds__(64) k_p2p_barrier(P2pRed pr, unsigned long long timeout_ticks, Scal *S)
{
    if (S->done) return;
    constexpr int d = kRedSlots - 1;
    for (int p = threadIdx.x; p < pr.nranks; p += 64)
        ll_store(pr.mail[p] + mail_index(pr.seq, pr.nranks, pr.rank, d), 0.0, pr.seq);
    for (int p = threadIdx.x; p < pr.nranks; p += 64) {
        double v;
        if (!ll_wait(pr.mail[pr.rank] + mail_index(pr.seq, pr.nranks, p, d), pr.seq, timeout_ticks, &v)) {
            S->comm_error = 1;
            S->done = 1;
        }
    }
}

void launch_p2p_barrier(const P2pRed &pr, unsigned long long timeout_ticks, Scal *S, hipStream_t st)
{
    BICG_LAUNCH(k_p2p_barrier, dim3(1), dim3(64), 0, st, pr, timeout_ticks, S);
}

// Second part of the transport self-test: the HALO pattern -- every rank stores `entries` values per
// round into the landing ring of every other rank and reads what the others stored into its own,
// for more rounds than the ring has slots (a reused slot must never be read with its old contents),
// with the ranks deliberately out of step and the solver's flow control (a token barrier every
// kHaloRing - 2 exchanges). Ring layout: [kHaloRing][source rank][entries][2 words].
__device__ __forceinline__ double ringtest_value(int rank, unsigned seq, int i)
{
    return (double)(rank * 1009 + i * 17 + 1) * 1.0000001 + (double)seq * 0.25;
}
__global__ void __launch_bounds__(kBlock) k_p2p_ringtest(P2pRed pr, llword *const *rings, int entries, unsigned seq0, int rounds,
                                                         unsigned bar_seq0, unsigned long long timeout_ticks, int *status)
{
    __shared__ int s_bad, s_timeout;
    const int P = pr.nranks, me = pr.rank;
    if (threadIdx.x == 0) { s_bad = 0; s_timeout = 0; }
    __syncthreads();
    for (int r = 0; r < rounds; ++r) {
        const unsigned seq = seq0 + (unsigned)r;
        const size_t slot = seq % kHaloRing;
        if (r % (kHaloRing - 2) == 0) {          // flow control, as in spmv(): nobody runs more than a ring ahead
            const unsigned bs = bar_seq0 + (unsigned)(r / (kHaloRing - 2));
            for (int p = threadIdx.x; p < P; p += kBlock)
                ll_store(pr.mail[p] + mail_index(bs, P, me, kRedSlots - 1), 0.0, bs);
            for (int p = threadIdx.x; p < P; p += kBlock) {
                double v;
                if (!ll_wait(pr.mail[me] + mail_index(bs, P, p, kRedSlots - 1), bs, timeout_ticks, &v)) s_timeout = 1;
            }
            __syncthreads();
        }
        if ((r + me) & 1) __builtin_amdgcn_s_sleep(127);     // keep the ranks out of step
        for (int t = threadIdx.x; t < P * entries; t += kBlock) {
            const int p = t / entries, i = t % entries;
            ll_store(rings[p] + ((slot * P + me) * entries + i) * 2, ringtest_value(me, seq, i), seq);
        }
        for (int t = threadIdx.x; t < P * entries; t += kBlock) {
            const int p = t / entries, i = t % entries;
            double v;
            if (!ll_wait(rings[me] + ((slot * P + p) * entries + i) * 2, seq, timeout_ticks, &v)) s_timeout = 1;
            else if (!(v == ringtest_value(p, seq, i))) s_bad = 1;
        }
        __syncthreads();
        if (s_timeout) break;
    }
    if (threadIdx.x == 0) {
        if (s_bad) atomicAdd(&status[0], 1);
        if (s_timeout) atomicAdd(&status[1], 1);
    }
}

void launch_p2p_ringtest(const P2pRed &pr, llword *const *rings, int entries, unsigned seq0, int rounds, unsigned bar_seq0,
                         unsigned long long timeout_ticks, int *status, hipStream_t st)
{
    BICG_LAUNCH(k_p2p_ringtest, dim3(1), dim3(kBlock), 0, st, pr, rings, entries, seq0, rounds, bar_seq0, timeout_ticks, status);
}

void launch_p2p_selftest(const P2pRed &pr, unsigned seq0, int rounds, unsigned long long timeout_ticks, int *status,
                         hipStream_t st)
{
    BICG_LAUNCH(k_p2p_selftest, dim3(1), dim3(kBlock), 0, st, pr, seq0, rounds, timeout_ticks, status);
}

void preload_exchange_kernels() { preload_kernel(k_apply); }

}  // namespace bicg
