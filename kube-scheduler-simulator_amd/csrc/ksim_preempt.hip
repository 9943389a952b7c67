// ksim_preempt.hip — PostFilter: DefaultPreemption's dry run on the device
// (upstream preemption.go / default_preemption.go, v1.26).
//
// After an unschedulable cycle, every node where preemption might help (the
// filter pass failed it at NodeResourcesFit or, for a pod with host ports, at
// NodePorts) runs SelectVictimsOnNode on its own thread: remove every bound pod
// of lower priority, check the pod fits, then reprieve the removed pods most
// important first (priority desc, start time asc), keeping each one the pod
// still fits beside.  "Fits" is NodeResourcesFit on the node's requests and,
// for a pod with NodePorts uses, no pod left on the node in any of its port
// classes: the thread keeps the node's count of each (at most KSIM_MAX_USES)
// and moves it with every pod it removes or adds back, from the bound pods'
// class contributions (ksim_set_bound_pod_adds).  The bound pods are
// held per node in importance order (CSR), so the lower-priority pods are a
// suffix of the node's range.  One block then keeps the first numCandidates
// candidates in nodeTree order (upstream scans from a random offset; offset 0
// here) and picks one by pickOneNodeForPreemption's criteria.
#include "ksim_device.h"
#include "ksim_internal.h"
#include "ksim_wave.h"

namespace ksim {

__device__ __forceinline__ void row_add_req(NodeRow& r, const int64_t* q, int sign, int n_scalar) {
  r.req_cpu += sign * q[0];
  r.req_mem += sign * q[1];
  r.req_eph += sign * q[2];
#pragma unroll
  for (int k = 0; k < KSIM_MAX_SCALAR; k++)
    if (k < n_scalar) r.req_sc[k] += sign * q[3 + k];
  r.num_pods += sign;
}

// The preemptor's NodePorts uses on one node: held[i] = pods on the node of
// use i's port class (0 for every other use).  cls[i] is the class of port
// use i, kNoPortClass elsewhere (no add carries it), block-uniform.
constexpr int32_t kNoPortClass = -2;
struct PortHold {
  int32_t held[KSIM_MAX_USES];
};
// NodeInfo.AddPod / RemovePod on the holdings: the adds [e0, e1) of one pod (or
// nominated group) that count into a class of the preemptor's
__device__ __forceinline__ void hold_add(PortHold& h, const int32_t (&cls)[KSIM_MAX_USES],
                                         const ksim_class_add* __restrict__ adds, int32_t e0, int32_t e1, int sign) {
  for (int32_t e = e0; e < e1; e++) {
    const ksim_class_add x = adds[e];
#pragma unroll
    for (int i = 0; i < KSIM_MAX_USES; i++)
      if (cls[i] == x.cls) h.held[i] += sign * x.count;
  }
}
// nodeports Filter on the holdings (node_port_conflict)
__device__ __forceinline__ bool hold_conflict(const PortHold& h) {
  bool hit = false;
#pragma unroll
  for (int i = 0; i < KSIM_MAX_USES; i++)
    if (h.held[i] > 0) hit = true;
  return hit;
}

// SelectVictimsOnNode of one potential node.  PORTS: the dry run re-runs
// NodePorts beside NodeResourcesFit (the preemptor has port uses and the
// profile filters on them); fit: the profile has NodeResourcesFit.
template <bool PORTS>
__device__ __forceinline__ void select_victims(const DevCluster& c, const ksim_pod& p, const ksim_topo_use* U,
                                               const DevPreempt& pre, int32_t node, int32_t prio, bool fit,
                                               uint32_t port_mask, PreemptNode& out) {
  const int32_t a = pre.off[node], b = pre.off[node + 1];
  int32_t j0 = a;
  while (j0 < b && pre.prio[j0] >= prio) j0++;       // lower priorities: the suffix [j0, b)
  for (int32_t j = a; j < j0; j++) pre.vflag[j] = 0;   // no stale flags from an earlier preemptor
  NodeRow r = load_row(c, node);
  const int32_t g = pre.nslot ? pre.nslot[node] : -1;
  if (g >= 0) {                                         // the nominated pods stay (pass 1)
    const int64_t* q = pre.nreq + (size_t)g * (KSIM_PREEMPT_REQ + 1);
    row_add_req(r, q, 1, c.n_scalar);
    r.num_pods += (int32_t)q[KSIM_PREEMPT_REQ] - 1;
  }
  int32_t cls[KSIM_MAX_USES];
  PortHold h;
  if (PORTS) {
#pragma unroll
    for (int i = 0; i < KSIM_MAX_USES; i++) {
      cls[i] = kNoPortClass;
      h.held[i] = 0;
      if ((port_mask >> i) & 1u) {
        cls[i] = load_use(U, i).cls;
        h.held[i] = (int32_t)class_count(c, cls[i], node);
      }
    }
    if (g >= 0) hold_add(h, cls, pre.gadds, pre.goff[g], pre.goff[g + 1], 1);
  }
  for (int32_t j = j0; j < b; j++) {
    row_add_req(r, pre.req + (size_t)j * KSIM_PREEMPT_REQ, -1, c.n_scalar);
    if (PORTS) hold_add(h, cls, pre.adds, pre.aoff[j], pre.aoff[j + 1], -1);
  }
  // the filters the dry run re-runs: 0 = the pod passes
  auto fails = [&]() -> bool {
    if ((!PORTS || fit) && fits_request(r, p, c.n_scalar, c.fit_ignore) != 0) return true;
    return PORTS && hold_conflict(h);
  };
  if (!fails()) {
    out.cand = 1;
    int32_t nv = 0, high = 0;
    int64_t sum = 0, early = INT64_MAX;
    for (int32_t j = j0; j < b; j++) {                 // reprievePod, most important first
      const int64_t* q = pre.req + (size_t)j * KSIM_PREEMPT_REQ;
      row_add_req(r, q, 1, c.n_scalar);
      if (PORTS) hold_add(h, cls, pre.adds, pre.aoff[j], pre.aoff[j + 1], 1);
      const bool victim = fails();
      pre.vflag[j] = victim;
      if (victim) {
        row_add_req(r, q, -1, c.n_scalar);
        if (PORTS) hold_add(h, cls, pre.adds, pre.aoff[j], pre.aoff[j + 1], -1);
        if (nv == 0) high = pre.prio[j];
        sum += (int64_t)pre.prio[j] + ((int64_t)INT32_MAX + 1);
        if (pre.prio[j] == high && pre.start[j] < early) early = pre.start[j];   // GetEarliestPodStartTime
        nv++;
      }
    }
    out.nv = nv;
    out.high = nv ? high : INT32_MIN;
    out.sum = sum;
    out.early = early;
  } else {
    for (int32_t j = j0; j < b; j++) pre.vflag[j] = 0;
  }
}

// Per node: SelectVictimsOnNode.  res[node] = {candidate, victims, highest
// victim priority, sum of (priority + 2^31), earliest start among the
// highest-priority victims}; vflag marks the victims (CSR order).  A potential
// node failed NodeResourcesFit or, for a preemptor with port uses (port_mask),
// NodePorts: the two filters that return Unschedulable and that the dry run
// re-runs.
__global__ __launch_bounds__(256) void k_preempt_nodes(DevCluster c, DevPods P, const DevState* __restrict__ st,
                                                       DevScratch s, DevPreempt pre, int32_t fit_index,
                                                       int32_t prio, int32_t port_index, uint32_t port_mask) {
  const int32_t node = blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= c.n) return;
  PreemptNode out{};
  out.cand = 0;
  const uint8_t f = s.fail[node];
  const bool potential = (fit_index >= 0 && f == (uint8_t)fit_index) || (port_mask && f == (uint8_t)port_index);
  out.potential = potential;
  if (potential) {
    const ksim_pod& p = P.pods[st->cursor];
    const ksim_topo_use* U = P.uses + p.use_first;
    if (port_mask)                                     // kernel argument: one uniform branch
      select_victims<true>(c, p, U, pre, node, prio, fit_index >= 0, port_mask, out);
    else
      select_victims<false>(c, p, U, pre, node, prio, true, 0u, out);
  }
  pre.res[node] = out;
}

// pickOneNodeForPreemption order: a is better than b
__device__ __forceinline__ bool better(const PreemptNode& a, int32_t na, const PreemptNode& b, int32_t nb) {
  if (nb < 0) return na >= 0;
  if (na < 0) return false;
  if (a.high != b.high) return a.high < b.high;
  if (a.sum != b.sum) return a.sum < b.sum;
  if (a.nv != b.nv) return a.nv < b.nv;
  if (a.early != b.early) return a.early > b.early;
  return na < nb;                                        // the first candidate in scan order
}

constexpr int kPickThreads = 1024;

// min_pct / min_abs: DefaultPreemptionArgs (calculateNumCandidates)
__global__ __launch_bounds__(kPickThreads) void k_preempt_pick(DevCluster c, DevPreempt pre, int32_t min_pct,
                                                               int32_t min_abs) {
  __shared__ int32_t sh[kPickThreads / 64];
  __shared__ PreemptNode s_best[kPickThreads];
  __shared__ int32_t s_node[kPickThreads];
  const int tid = threadIdx.x;
  const int32_t N = c.n, chunk = (N + kPickThreads - 1) / kPickThreads;
  const int32_t lo = min(N, tid * chunk), hi = min(N, lo + chunk);
  int32_t npot = 0, ncand = 0;
  for (int32_t x = lo; x < hi; x++) {
    npot += pre.res[x].potential;
    ncand += pre.res[x].cand;
  }
  // GetOffsetAndNumCandidates over the potential nodes; candidates are kept
  // in nodeTree order until that many were found
  int32_t total_pot, cexcl, total_cand;
  {
    const int lane = tid & 63, w = tid >> 6;
    int32_t x = npot, y = ncand;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int32_t a = __shfl_up(x, d, 64), b = __shfl_up(y, d, 64);
      if (lane >= d) {
        x += a;
        y += b;
      }
    }
    __syncthreads();
    if (lane == 63) sh[w] = x;
    __syncthreads();
    int32_t base = 0, tot = 0;
    for (int i = 0; i < kPickThreads / 64; i++) {
      if (i < w) base += sh[i];
      tot += sh[i];
    }
    total_pot = tot;
    __syncthreads();
    if (lane == 63) sh[w] = y;
    __syncthreads();
    base = 0;
    tot = 0;
    for (int i = 0; i < kPickThreads / 64; i++) {
      if (i < w) base += sh[i];
      tot += sh[i];
    }
    cexcl = base + y - ncand;
    total_cand = tot;
  }
  int32_t want = total_pot * min_pct / 100;
  if (want < min_abs) want = min_abs;
  if (want > total_pot) want = total_pot;
  PreemptNode best{};
  int32_t best_node = -1, rank = cexcl;
  for (int32_t x = lo; x < hi; x++) {
    const PreemptNode& r = pre.res[x];
    if (!r.cand) continue;
    if (rank < want && better(r, x, best, best_node)) {
      best = r;
      best_node = x;
    }
    rank++;
  }
  s_best[tid] = best;
  s_node[tid] = best_node;
  __syncthreads();
  for (int stride = kPickThreads / 2; stride > 0; stride >>= 1) {
    if (tid < stride && better(s_best[tid + stride], s_node[tid + stride], s_best[tid], s_node[tid])) {
      s_best[tid] = s_best[tid + stride];
      s_node[tid] = s_node[tid + stride];
    }
    __syncthreads();
  }
  if (tid == 0) {
    pre.pick[0] = s_node[0];
    pre.pick[1] = s_node[0] >= 0 ? s_best[0].nv : 0;
    pre.pick[2] = total_pot;
    pre.pick[3] = total_cand < want ? total_cand : want;
  }
}

void launch_preempt(const LaunchArgs& a, const DevPreempt& pre, int32_t fit_index, int32_t prio,
                    hipStream_t stream, bool filter, int32_t port_index, uint32_t port_mask) {
  const int blocks = (a.c.n + 255) / 256;
  if (filter) launch_filter_only(a, stream);             // the filter statuses of every node
  if (port_index < 0) port_mask = 0;                     // no NodePorts in the profile: port uses are ignored
  k_preempt_nodes<<<blocks, 256, 0, stream>>>(a.c, a.P, a.st, a.s, pre, fit_index, prio, port_index, port_mask);
  k_preempt_pick<<<1, kPickThreads, 0, stream>>>(a.c, pre, a.prof.preempt_min_pct, a.prof.preempt_min_abs);
}

}  // namespace ksim
