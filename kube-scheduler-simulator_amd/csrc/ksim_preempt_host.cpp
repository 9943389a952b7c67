// ksim_preempt_host.cpp — the host side of DefaultPreemption (the bound-pod
// table, the lists set on its rows, the dry run behind the ksim_preempt*
// entry points; kernels in ksim_preempt.hip) and of ksim_match_terms
// (ksim_match.hip).
#include <algorithm>
#include <cstring>

#include "ksim_host.h"

using namespace ksim_host;

// A pod's KSIM_USE_VOLUME uses (host arrays, the ABI form).
static bool has_volume_use(const ksim_pod_set* ps, int32_t i) {
  if (!ps || !ps->pods || !ps->uses || i < 0 || i >= ps->n_pods) return false;
  const ksim_pod& p = ps->pods[i];
  if (p.use_first < 0 || p.use_count < 0 || (int64_t)p.use_first + p.use_count > ps->n_uses) return false;
  for (int32_t k = 0; k < p.use_count; k++)
    if (ps->uses[p.use_first + k].kind == KSIM_USE_VOLUME) return true;
  return false;
}

// ---- PostFilter: DefaultPreemption (ksim_preempt.hip) ------------------------------
extern "C" int ksim_set_bound_pods(ksim_handle* h, const ksim_bound_pods* b) {
  int rc = ensure_ready(h);
  if (rc) return rc;
  if (!b || b->n < 0 || (b->n > 0 && (!b->node || !b->priority || !b->start_time || !b->req)))
    return set_err(h, KSIM_E_INVALID, "bad bound-pod table");
  const int32_t N = h->dc.n, n = b->n;
  for (int32_t i = 0; i < n; i++)
    if (b->node[i] < 0 || b->node[i] >= N) return set_err(h, KSIM_E_INVALID, "bound pod on a node out of range");
  // per node, util.MoreImportantPod order (priority desc, start asc), then table order
  std::vector<int32_t> ix((size_t)n);
  for (int32_t i = 0; i < n; i++) ix[i] = i;
  std::sort(ix.begin(), ix.end(), [&](int32_t x, int32_t y) {
    if (b->node[x] != b->node[y]) return b->node[x] < b->node[y];
    if (b->priority[x] != b->priority[y]) return b->priority[x] > b->priority[y];
    if (b->start_time[x] != b->start_time[y]) return b->start_time[x] < b->start_time[y];
    return x < y;
  });
  std::vector<int32_t> off((size_t)N + 1, 0), prio((size_t)std::max(n, 1));
  std::vector<int64_t> start((size_t)std::max(n, 1)), req((size_t)std::max(n, 1) * KSIM_PREEMPT_REQ);
  for (int32_t i = 0; i < n; i++) off[b->node[i] + 1]++;
  for (int32_t v = 0; v < N; v++) off[v + 1] += off[v];
  for (int32_t k = 0; k < n; k++) {
    const int32_t i = ix[k];
    prio[k] = b->priority[i];
    start[k] = b->start_time[i];
    for (int q = 0; q < KSIM_PREEMPT_REQ; q++) req[(size_t)k * KSIM_PREEMPT_REQ + q] = b->req[(size_t)i * KSIM_PREEMPT_REQ + q];
  }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // the old table goes whole: the lists belonged to its rows, ksim_preempt_many's slabs are sized by it
  h->bound = BoundPods{};
  DevPreempt d{};
  if ((rc = h->bound.bufs.alloc(h, d.off, 4 * off.size(), off.data())) ||
      (rc = h->bound.bufs.alloc(h, d.prio, 4 * prio.size(), prio.data())) ||
      (rc = h->bound.bufs.alloc(h, d.start, 8 * start.size(), start.data())) ||
      (rc = h->bound.bufs.alloc(h, d.req, 8 * req.size(), req.data())) ||
      (rc = h->bound.bufs.alloc(h, d.vflag, (size_t)std::max(n, 1))) ||
      (rc = h->bound.bufs.alloc(h, d.res, sizeof(PreemptNode) * (size_t)N)) ||
      (rc = h->bound.bufs.alloc(h, d.pick, 32)) ||
      (rc = h->bound.bufs.alloc(h, d.nslot, 4 * (size_t)std::max(N, 1))))
    return rc;
  HIPCHK(h, hipMemsetAsync(d.nslot, 0xff, 4 * (size_t)std::max(N, 1), h->stream));   // -1: no group
  d.nreq = nullptr;
  if ((rc = h->bound.bufs.alloc(h, d.afftot, 8 * (size_t)KSIM_MAX_USES)) ||
      (rc = h->bound.bufs.alloc(h, h->bound.smin, 8 * 3 * (size_t)KSIM_MAX_USES)) ||
      (rc = h->bound.bufs.alloc(h, h->bound.dindex, 4 * (size_t)std::max(n, 1), n > 0 ? ix.data() : nullptr)))
    return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->bound.d = d;
  h->bound.index = ix;
  h->bound.n = n;
  // what ksim_preempt_commit checks its rows against
  h->bound.row_node.assign(b->node, b->node + n);
  h->bound.row_req.assign(b->req, b->req + (size_t)n * KSIM_PREEMPT_REQ);
  h->bound.dead.assign((size_t)n, 0);
  h->bound.live = n;
  for (int32_t v = 0; v < N; v++) h->bound.maxrow = std::max(h->bound.maxrow, off[v + 1] - off[v]);
  return KSIM_OK;
}

// The lists set on the bound-pod table's rows (ksim_set_bound_pod_adds, _pdbs,
// _volumes) arrive as a CSR over the caller's rows.  Its offsets: monotone,
// from off[0] >= 0 (from_zero: from 0), with the entries there when the list
// is not empty.  fn: the calling function, as the error texts name it.
static int bound_csr_check(ksim_handle* h, const std::string& fn, const int32_t* off, bool have_entries,
                           const char* what, bool from_zero) {
  const int32_t n = h->bound.n;
  if (!off || (from_zero ? off[0] != 0 : off[0] < 0))
    return set_err(h, KSIM_E_INVALID, fn + (from_zero ? ": bad offsets (they start at 0)" : ": bad offsets"));
  for (int32_t i = 0; i < n; i++)
    if (off[i + 1] < off[i]) return set_err(h, KSIM_E_INVALID, fn + ": offsets not monotone");
  if (off[n] > off[0] && !have_entries) return set_err(h, KSIM_E_INVALID, fn + ": " + what + " missing");
  return KSIM_OK;
}

// ... and, every entry validated by the caller: the rows go into the table's
// per-node importance order (CSR position k = caller row bound.index[k]; conv
// makes the device's entry of the caller's), the old list is freed (every dry
// run ends synchronized: nothing reads it) and the new one uploaded, and
// published once the copies have read this call's vectors.  off == null only
// clears the list.  extra: one more int32 array that goes with the list (the
// budgets' allowed counts).  After a ksim_preempt_commit the caller's CSR still
// spans all its rows; the table's positions are the rows left, so an evicted
// row's entries are passed over (the host's bound.index is compacted here, where
// the work is O(rows) anyway).  list: its owner (the entries uploaded counted there); alt_off / alt_ent:
// the commit's second buffers of this list, which go with the old ones.
template <class E, class In, class Conv>
static int bound_csr_set(ksim_handle* h, BoundList& list, const int32_t* off, const In* in, Conv conv,
                         const int32_t*& d_off, const E*& d_ent, int32_t*& alt_off, E*& alt_ent,
                         const int32_t* extra = nullptr, size_t n_extra = 0, const int32_t** d_extra = nullptr) {
  if (h->bound.index_stale) {
    h->bound.index.erase(std::remove_if(h->bound.index.begin(), h->bound.index.end(),
                                      [&](int32_t i) { return h->bound.dead[i] != 0; }),
                       h->bound.index.end());
    h->bound.index_stale = false;
  }
  const int32_t n = h->bound.live;
  std::vector<int32_t> poff((size_t)n + 1, 0);
  std::vector<E> perm;
  if (off) {
    perm.reserve((size_t)(off[h->bound.n] - off[0]));
    for (int32_t k = 0; k < n; k++) {
      const int32_t i = h->bound.index[k];
      for (int32_t e = off[i]; e < off[i + 1]; e++) perm.push_back(conv(in[e]));
      poff[(size_t)k + 1] = (int32_t)perm.size();
    }
  }
  HIPCHK(h, hipSetDevice(h->device));
  list = BoundList{};
  d_off = nullptr;
  d_ent = nullptr;
  alt_off = nullptr;
  alt_ent = nullptr;
  if (d_extra) *d_extra = nullptr;
  if (!off) return KSIM_OK;
  const int32_t *po = nullptr, *px = nullptr;
  const E* pe = nullptr;
  int rc;
  if ((rc = list.bufs.alloc(h, po, 4 * poff.size(), poff.data())) ||
      (rc = list.bufs.alloc(h, pe, sizeof(E) * perm.size(), perm.data())) ||
      (d_extra && (rc = list.bufs.alloc(h, px, 4 * n_extra, extra))))
    return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));   // the copies read this call's vectors
  d_off = po;
  d_ent = pe;
  list.ents = perm.size();
  if (d_extra) *d_extra = px;
  return KSIM_OK;
}

extern "C" int ksim_set_bound_pod_adds(ksim_handle* h, const int32_t* off, const ksim_class_add* adds) {
  if (!h) return KSIM_E_INVALID;
  if (!h->bound.d.off) return set_err(h, KSIM_E_INVALID, "ksim_set_bound_pod_adds: ksim_set_bound_pods first");
  if (const int rc = bound_csr_check(h, "ksim_set_bound_pod_adds", off, adds != nullptr, "adds", false)) return rc;
  for (int32_t e = off[0]; e < off[h->bound.n]; e++)
    if (adds[e].cls < 0 || adds[e].cls >= h->dc.n_classes)
      return set_err(h, KSIM_E_INVALID, "ksim_set_bound_pod_adds: class out of range");
  return bound_csr_set(h, h->bound.add, off, adds, [](const ksim_class_add& a) { return a; }, h->bound.d.aoff,
                       h->bound.d.adds, h->bound.alt.aoff2, h->bound.alt.adds2);
}

extern "C" int ksim_set_bound_pod_pdbs(ksim_handle* h, int32_t n_pdbs, const int32_t* allowed, const int32_t* off,
                                       const int32_t* ids) {
  if (!h) return KSIM_E_INVALID;
  if (!h->bound.d.off) return set_err(h, KSIM_E_INVALID, "ksim_set_bound_pod_pdbs: ksim_set_bound_pods first");
  if (n_pdbs < 0) return set_err(h, KSIM_E_INVALID, "ksim_set_bound_pod_pdbs: negative budget count");
  if (n_pdbs > 0) {
    // the offsets start at 0 here, and the allowed counts are as much a part of them as the array itself
    if (const int rc = bound_csr_check(h, "ksim_set_bound_pod_pdbs", allowed ? off : nullptr, ids != nullptr, "ids", true))
      return rc;
    std::vector<int32_t> last((size_t)n_pdbs, -1);   // the last row that named the budget
    for (int32_t i = 0; i < h->bound.n; i++)
      for (int32_t e = off[i]; e < off[i + 1]; e++) {
        if (ids[e] < 0 || ids[e] >= n_pdbs)
          return set_err(h, KSIM_E_INVALID, "ksim_set_bound_pod_pdbs: budget id out of range");
        if (last[ids[e]] == i) return set_err(h, KSIM_E_INVALID, "ksim_set_bound_pod_pdbs: a budget twice in one row");
        last[ids[e]] = i;
      }
  }
  // n_pdbs == 0 clears: the dry run takes the forms without budgets
  return bound_csr_set(h, h->bound.pdb, n_pdbs > 0 ? off : nullptr, ids, [](int32_t id) { return id; }, h->bound.d.poff,
                       h->bound.d.pids, h->bound.alt.poff2, h->bound.alt.pids2, allowed, (size_t)n_pdbs,
                       &h->bound.d.pallowed);
}

extern "C" int ksim_set_bound_pod_volumes(ksim_handle* h, const int32_t* off, const ksim_topo_use* uses) {
  if (!h) return KSIM_E_INVALID;
  if (!h->bound.d.off) return set_err(h, KSIM_E_INVALID, "ksim_set_bound_pod_volumes: ksim_set_bound_pods first");
  if (!h->dc.vol_nf)
    return set_err(h, KSIM_E_INVALID, "ksim_set_bound_pod_volumes: no volume table (ksim_set_volume_limits)");
  if (const int rc = bound_csr_check(h, "ksim_set_bound_pod_volumes", off, uses != nullptr, "uses", false)) return rc;
  for (int32_t e = off[0]; e < off[h->bound.n]; e++) {
    const ksim_topo_use& u = uses[e];
    if (u.kind != KSIM_USE_VOLUME)
      return set_err(h, KSIM_E_INVALID, "ksim_set_bound_pod_volumes: a use that is no KSIM_USE_VOLUME");
    if (u.col >= h->dc.vol_nf) return set_err(h, KSIM_E_INVALID, "ksim_set_bound_pod_volumes: family out of range");
    if (u.cls < -1 || u.cls >= h->dc.n_classes)
      return set_err(h, KSIM_E_INVALID, "ksim_set_bound_pod_volumes: class out of range");
    if (u.cls < 0 ? u.arg < 1 : u.arg != 1)
      return set_err(h, KSIM_E_INVALID, "ksim_set_bound_pod_volumes: bad volume use count");
  }
  return bound_csr_set(h, h->bound.vol, off, uses,
                       [](const ksim_topo_use& u) { return VolHold{u.cls, (int32_t)u.col, u.arg}; }, h->bound.voff,
                       h->bound.vols, h->bound.alt.voff2, h->bound.alt.vols2);
}

extern "C" int ksim_preempt(ksim_handle* h, const ksim_pod_set* ps, int32_t pod_index, int32_t priority,
                            ksim_preempt_out* out) {
  return ksim_preempt_nominated(h, ps, pod_index, priority, nullptr, 0, nullptr, nullptr, nullptr, out);
}

// The entry point a dry run came through (plain: ksim_preempt / _nominated), which says what it accepts:
//   a KSIM_USE_VOLUME use     through `volumes` (beside no affinity or spread use) and `full`;
//   a KSIM_USE_PTS_HARD use   through `spread` and `full`.
// Through `full` a preemptor with volume groups also has VolumeBinding / VolumeZone re-run.
enum class PreemptEntry { plain, spread, volumes, full };
struct NominatedGroups {   // of one call: pods [first[k], first[k] + count[k]) of ps on node nodes[k], k < n
  const ksim_pod_set* ps;
  int32_t n;
  const int32_t *nodes, *first, *count;
};

static int preempt_check_args(ksim_handle* h, const ksim_pod_set* ps, int32_t pod_index, const NominatedGroups& ng,
                              const ksim_preempt_out* out, PreemptEntry entry) {
  int rc;
  if (!ps || !out || pod_index < 0 || pod_index >= ps->n_pods || !ps->pods)
    return set_err(h, KSIM_E_INVALID, "bad pod set / index");
  if (ng.n < 0 || (ng.n > 0 && (!ng.ps || !ng.ps->pods || !ng.nodes || !ng.first || !ng.count)))
    return set_err(h, KSIM_E_INVALID, "bad nominated-node groups");
  if (has_volume_use(ps, pod_index) && entry != PreemptEntry::volumes && entry != PreemptEntry::full)
    return set_err(h, KSIM_E_UNSUPPORTED, "preemption for pods with a KSIM_USE_VOLUME use (the dry run does not "
                                          "re-run the node volume limit plugins)");
  std::vector<uint8_t> seen((size_t)std::max(h->dc.n, 1), 0);
  for (int32_t k = 0; k < ng.n; k++) {
    if (ng.nodes[k] < 0 || ng.nodes[k] >= h->dc.n || seen[ng.nodes[k]])
      return set_err(h, KSIM_E_INVALID, "nominated node out of range or repeated");
    seen[ng.nodes[k]] = 1;
    if (ng.count[k] < 0 || ng.first[k] < 0 || ng.first[k] + ng.count[k] > ng.ps->n_pods)
      return set_err(h, KSIM_E_INVALID, "nominated pod range out of the pod set");
    for (int32_t j = ng.first[k]; j < ng.first[k] + ng.count[k]; j++)
      if ((rc = validate_pod(h, ng.ps, j))) return rc;
  }
  if (!h->bound.d.off) return set_err(h, KSIM_E_INVALID, "ksim_set_bound_pods first");
  if (is_sharded(h)) return set_err(h, KSIM_E_UNSUPPORTED, "preemption runs on unsharded handles");
  if (prof_has_filter(h->prof, KSIM_PL_NETWORK_BANDWIDTH))
    return set_err(h, KSIM_E_UNSUPPORTED, "preemption dry runs re-run Fit only, not NetworkBandwidth");
  if (ps->pods[pod_index].flags & KSIM_POD_NODE_NAMES)
    return set_err(h, KSIM_E_UNSUPPORTED, "preemption for pods a PreFilterResult restricts");
  return validate_pod(h, ps, pod_index);
}

// Which uses does the dry run read?  It re-runs NodeResourcesFit, NodePorts,
// InterPodAffinity, PodTopologySpread and the node volume limit plugins where
// the profile filters on them.  A use that no Filter reads (ScheduleAnyway
// spread, InterPodAffinity scores, ImageLocality) or whose filter the profile
// lacks is in none of the plan's masks.
static int preempt_plan(ksim_handle* h, const ksim_pod_set* ps, int32_t pod_index, int32_t priority,
                        PreemptEntry entry, PreemptPlan& q) {
  q = PreemptPlan{};
  q.fit = q.port = q.ipa = q.pts = -1;
  q.prio = priority, q.smin = h->bound.smin;
  for (int f = 0; f < h->prof.n_filter; f++) {
    if (h->prof.filter[f] == KSIM_PL_NODE_RESOURCES_FIT) q.fit = f;
    if (h->prof.filter[f] == KSIM_PL_NODE_PORTS) q.port = f;
    if (h->prof.filter[f] == KSIM_PL_INTER_POD_AFFINITY) q.ipa = f;
    if (h->prof.filter[f] == KSIM_PL_POD_TOPOLOGY_SPREAD) q.pts = f;
  }
  const ksim_pod& pp = ps->pods[pod_index];
  const ksim_topo_use* uses = ps->uses + pp.use_first;
  const bool full = entry == PreemptEntry::full, vol_form = has_volume_use(ps, pod_index);
  for (int32_t k = 0; k < pp.use_count && vol_form && !full; k++) {
    static const char* const kNames[] = {"KSIM_USE_PTS_HARD", nullptr, "KSIM_USE_IPA_EXISTING_ANTI",
                                         "KSIM_USE_IPA_AFFINITY", "KSIM_USE_IPA_ANTI"};
    if (uses[k].kind <= KSIM_USE_IPA_ANTI && kNames[uses[k].kind])
      return set_err(h, KSIM_E_UNSUPPORTED, std::string("preemption for pods with a KSIM_USE_VOLUME use and a ") +
                                                kNames[uses[k].kind] + " use (the volume form moves no domain counts)");
  }
  for (int32_t k = 0; k < pp.use_count && entry != PreemptEntry::spread && !full; k++)
    if (uses[k].kind == KSIM_USE_PTS_HARD)   // (the older entry points' callers fall back on that code)
      return set_err(h, KSIM_E_UNSUPPORTED, "preemption for pods with a KSIM_USE_PTS_HARD use (its dry run needs the "
                                            "victims' domains: ksim_preempt_spread)");
  for (int32_t k = 0; k < pp.use_count; k++) {
    const uint8_t kind = uses[k].kind;
    if (kind == KSIM_USE_NODE_PORT && q.port >= 0) q.ports |= 1u << k;
    if (kind == KSIM_USE_IPA_AFFINITY && q.ipa >= 0) q.aff |= 1u << k;
    if (kind == KSIM_USE_IPA_ANTI && q.ipa >= 0) q.anti |= 1u << k;
    if (kind == KSIM_USE_IPA_EXISTING_ANTI && q.ipa >= 0) q.exist |= 1u << k;
    if (kind == KSIM_USE_PTS_HARD && q.pts >= 0) q.hard |= 1u << k;
  }
  const bool dom = q.reads_domains();
  if (q.hard && !h->bound.d.aoff)
    return set_err(h, KSIM_E_INVALID, "ksim_preempt_spread for a pod with DoNotSchedule spread: "
                                      "ksim_set_bound_pod_adds first (after ksim_set_bound_pods), every class");
  if (q.ports && !dom && !h->bound.d.aoff)
    return set_err(h, KSIM_E_INVALID, "preemption for a pod with host ports: ksim_set_bound_pod_adds first "
                                      "(after ksim_set_bound_pods)");
  if (vol_form && !h->bound.voff)
    return set_err(h, KSIM_E_INVALID, "preemption for a pod with a KSIM_USE_VOLUME use: ksim_set_bound_pod_volumes "
                                      "first (after ksim_set_bound_pods)");
  // what the profile's limit plugins read of the pod (validate_pod checked the families)
  PreemptVol& vm = q.vol;
  vm.at = 0xffffffffu;
  if (vol_form) {
    vm.voff = h->bound.voff;
    vm.vols = h->bound.vols;
    for (int f = 0; f < h->prof.n_filter; f++) {
      const int32_t k = h->prof.filter[f] - KSIM_PL_EBS_LIMITS;
      if (k >= 0 && k < 4) vm.at = (vm.at & ~(255u << (8 * k))) | ((uint32_t)f << (8 * k));
    }
    for (int32_t k = 0; k < pp.use_count; k++) {
      const ksim_topo_use& u = uses[k];
      if (u.kind != KSIM_USE_VOLUME) continue;
      const uint32_t pl = (h->dc.vol_plug >> (4 * u.col)) & 15u;
      if (((vm.at >> (8 * pl)) & 255u) == 255u) continue;   // its plugin is not in the filter list
      vm.uses |= 1u << k;
      vm.fams |= 1u << u.col;
      if (pl == (uint32_t)(KSIM_PL_NODE_VOLUME_LIMITS - KSIM_PL_EBS_LIMITS)) vm.csi |= 1u << u.col;
    }
  }
  if (dom && !h->bound.d.aoff)
    return set_err(h, KSIM_E_INVALID, "preemption for a pod with required pod (anti-)affinity: "
                                      "ksim_set_bound_pod_adds first (after ksim_set_bound_pods), every class");
  // the static volume filters of a preemptor with groups
  q.vb = full && pp.vb_count > 0 && prof_has_filter(h->prof, KSIM_PL_VOLUME_BINDING);
  q.vz = full && pp.vz_count > 0 && prof_has_filter(h->prof, KSIM_PL_VOLUME_ZONE);
  return KSIM_OK;
}

// The status pass: the per-pod cycle's filter phase.  For a pod with uses
// (topo) its PreFilter pass runs first; the domain tables and topology flags it
// fills are zero between cycles (k_select / k_bind re-zero them in a whole
// cycle).  keep: a form with a row side reads the last pass's tables, so the
// caller re-zeroes them after the node kernel.
static int preempt_rezero(ksim_handle* h) {
  if (h->sc.dom) HIPCHK(h, hipMemsetAsync(h->sc.dom, 0, 8 * (size_t)KSIM_MAX_USES * h->dc.vmax, h->stream));
  HIPCHK(h, hipMemsetAsync(&h->st->topo_flags, 0, sizeof(uint32_t), h->stream));
  return KSIM_OK;
}
static int preempt_filter_pass(ksim_handle* h, const LaunchArgs& a, bool topo, bool keep) {
  launch_filter_only(a, h->stream, topo);
  HIPCHK(h, hipGetLastError());
  return topo && !keep ? preempt_rezero(h) : KSIM_OK;
}

// The statuses the dry run starts from (s.fail): pass 1 of each grouped node,
// its nominated pods assumed on it, then every node as is.  The groups'
// requests, class contributions and volume holdings are uploaded for the sides
// that move them, and pre.nslot names each grouped node's group until the caller clears it.
static int preempt_statuses(ksim_handle* h, const LaunchArgs& a, const NominatedGroups& ng, bool topo,
                            PreemptPlan& plan, DevPreempt& pre) {
  int rc;
  const ksim_pod_set* nps = ng.ps;
  const int32_t n_groups = ng.n, *gnodes = ng.nodes, *first = ng.first, *count = ng.count;
  const bool dom_form = plan.reads_domains(), adds_form = plan.ports || dom_form, vol_form = plan.vol.voff != nullptr;
  std::vector<uint8_t> gfail((size_t)std::max(n_groups, 1), KSIM_PASSED);
  std::vector<int64_t> nreq((size_t)std::max(n_groups, 1) * (KSIM_PREEMPT_REQ + 1), 0);
  std::vector<int32_t> goff((size_t)n_groups + 1, 0);    // the groups' class contributions (CSR)
  std::vector<ksim_class_add> gadds;
  std::vector<int32_t> gvoff((size_t)n_groups + 1, 0);   // and their volume holdings, for the volume side
  std::vector<VolHold> gvols;
  auto bind_group = [&](int32_t k, int sign) -> int {
    for (int32_t j = first[k]; j < first[k] + count[k]; j++) {
      DevPods Q;
      int r;
      if ((r = upload_single(h, nps, j, Q, h->nom_arena))) return r;
      launch_assume(h->dc, Q, 0, gnodes[k], sign, h->stream);
      HIPCHK(h, hipGetLastError());
    }
    return KSIM_OK;
  };
  for (int32_t k = 0; k < n_groups; k++) {                // pass 1 of each grouped node
    if ((rc = bind_group(k, 1))) return rc;
    if ((rc = preempt_filter_pass(h, a, topo, false))) return rc;
    HIPCHK(h, hcopy(h, &gfail[k], h->sc.fail + gnodes[k], 1, hipMemcpyDeviceToHost));
    if ((rc = bind_group(k, -1))) return rc;
    int64_t* q = nreq.data() + (size_t)k * (KSIM_PREEMPT_REQ + 1);
    for (int32_t j = first[k]; j < first[k] + count[k]; j++) {
      const ksim_pod& x = nps->pods[j];
      q[0] += x.req_cpu;
      q[1] += x.req_mem;
      q[2] += x.req_eph;
      for (int c = 0; c < KSIM_MAX_SCALAR; c++) q[3 + c] += x.scalar_req[c];
      if (adds_form && x.add_count > 0) gadds.insert(gadds.end(), nps->adds + x.add_first, nps->adds + x.add_first + x.add_count);
      for (int32_t e = 0; e < x.use_count && vol_form; e++) {
        const ksim_topo_use& u = nps->uses[x.use_first + e];
        if (u.kind == KSIM_USE_VOLUME) gvols.push_back({u.cls, (int32_t)u.col, u.arg});
      }
    }
    q[KSIM_PREEMPT_REQ] = count[k];
    goff[(size_t)k + 1] = (int32_t)gadds.size();
    gvoff[(size_t)k + 1] = (int32_t)gvols.size();
  }
  if (n_groups > 0) {
    h->bound.nom_bufs.clear();
    if ((rc = h->bound.nom_bufs.alloc(h, pre.nreq, 8 * nreq.size(), nreq.data()))) return rc;
    if (adds_form) {                                       // the groups' holdings stay on their nodes too
      if ((rc = h->bound.nom_bufs.alloc(h, pre.goff, 4 * goff.size(), goff.data())) ||
          (rc = h->bound.nom_bufs.alloc(h, pre.gadds, sizeof(ksim_class_add) * gadds.size(), gadds.data())))
        return rc;
    }
    if (vol_form) {
      if ((rc = h->bound.nom_bufs.alloc(h, plan.vol.gvoff, 4 * gvoff.size(), gvoff.data())) ||
          (rc = h->bound.nom_bufs.alloc(h, plan.vol.gvols, sizeof(VolHold) * gvols.size(), gvols.data())))
        return rc;
    }
  }
  if ((rc = preempt_filter_pass(h, a, topo, dom_form))) return rc;   // every node as is
  for (int32_t k = 0; k < n_groups; k++) {
    // a grouped node's status: pass 1's unless it passed (then pass 2's, as is)
    if (gfail[k] != KSIM_PASSED) {
      gfail[k] &= (uint8_t)~kFailError;
      HIPCHK(h, hipMemcpyAsync(h->sc.fail + gnodes[k], &gfail[k], 1, hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(pre.nslot + gnodes[k], &k, 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));          // k and gfail[k] are host stack / vector slots
  }
  return KSIM_OK;
}

// The pick, and the nominated node's victims in the dry run's list order: the
// victims violating a PDB, then the others, each in CSR order.
static int preempt_read_back(ksim_handle* h, ksim_preempt_out* out) {
  int32_t pick[5];
  HIPCHK(h, hipMemcpyAsync(pick, h->bound.d.pick, sizeof(pick), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  out->nominated = pick[0];
  out->n_victims = pick[1];
  out->n_potential = pick[2];
  out->n_candidates = pick[3];
  out->n_pdb_violations = pick[4];
  if (pick[0] >= 0 && out->victims && out->victims_cap > 0) {
    std::vector<int32_t> off(2);
    HIPCHK(h, hcopy(h, off.data(), h->bound.d.off + pick[0], 8, hipMemcpyDeviceToHost));
    std::vector<uint8_t> flag((size_t)std::max(off[1] - off[0], 1));
    if (off[1] > off[0])
      HIPCHK(h, hcopy(h, flag.data(), h->bound.d.vflag + off[0], (size_t)(off[1] - off[0]), hipMemcpyDeviceToHost));
    // the positions' caller rows: the host's copy, or after a ksim_preempt_commit (which leaves
    // that one uncompacted) the node's range of the device's
    std::vector<int32_t> moved;
    const int32_t* index = h->bound.index.data() + off[0];
    if (h->bound.index_stale && off[1] > off[0]) {
      moved.resize((size_t)(off[1] - off[0]));
      HIPCHK(h, hcopy(h, moved.data(), h->bound.dindex + off[0], 4 * moved.size(), hipMemcpyDeviceToHost));
      index = moved.data();
    }
    int32_t k = 0;
    for (const uint8_t want : {(uint8_t)(1 | kPreemptViolating), (uint8_t)1})
      for (int32_t j = off[0]; j < off[1] && k < out->victims_cap; j++)
        if (flag[j - off[0]] == want) out->victims[k++] = index[j - off[0]];
  }
  return KSIM_OK;
}

// The dry run behind the four entry points.
static int preempt_run(ksim_handle* h, const ksim_pod_set* ps, int32_t pod_index, int32_t priority,
                       const NominatedGroups& ng, ksim_preempt_out* out, PreemptEntry entry) {
  int rc = ensure_ready(h);
  if (rc) return rc;
  PreemptPlan plan;
  if ((rc = preempt_check_args(h, ps, pod_index, ng, out, entry)) ||
      (rc = preempt_plan(h, ps, pod_index, priority, entry, plan)))
    return rc;
  HIPCHK(h, hipSetDevice(h->device));
  DevPods P;
  if ((rc = upload_single(h, ps, pod_index, P))) return rc;
  if ((rc = set_run(h, 0, 1))) return rc;
  const LaunchArgs a = make_args(h, P, nullptr);
  DevPreempt pre = h->bound.d;
  if ((rc = preempt_statuses(h, a, ng, ps->pods[pod_index].use_count > 0, plan, pre))) return rc;
  launch_preempt(a, pre, plan, h->stream);
  HIPCHK(h, hipGetLastError());
  if (plan.reads_domains() && (rc = preempt_rezero(h))) return rc;   // the tables the node kernel read
  static const int32_t kNoGroup = -1;
  for (int32_t k = 0; k < ng.n; k++)
    HIPCHK(h, hipMemcpyAsync(pre.nslot + ng.nodes[k], &kNoGroup, 4, hipMemcpyHostToDevice, h->stream));
  return preempt_read_back(h, out);
}

extern "C" int ksim_preempt_nominated(ksim_handle* h, const ksim_pod_set* ps, int32_t pod_index, int32_t priority,
                                      const ksim_pod_set* nps, int32_t n_groups, const int32_t* gnodes,
                                      const int32_t* first, const int32_t* count, ksim_preempt_out* out) {
  return preempt_run(h, ps, pod_index, priority, {nps, n_groups, gnodes, first, count}, out, PreemptEntry::plain);
}

extern "C" int ksim_preempt_volumes(ksim_handle* h, const ksim_pod_set* ps, int32_t pod_index, int32_t priority,
                                    const ksim_pod_set* nps, int32_t n_groups, const int32_t* gnodes,
                                    const int32_t* first, const int32_t* count, ksim_preempt_out* out) {
  return preempt_run(h, ps, pod_index, priority, {nps, n_groups, gnodes, first, count}, out, PreemptEntry::volumes);
}

extern "C" int ksim_preempt_full(ksim_handle* h, const ksim_pod_set* ps, int32_t pod_index, int32_t priority,
                                 const ksim_pod_set* nps, int32_t n_groups, const int32_t* gnodes,
                                 const int32_t* first, const int32_t* count, ksim_preempt_out* out) {
  return preempt_run(h, ps, pod_index, priority, {nps, n_groups, gnodes, first, count}, out, PreemptEntry::full);
}

extern "C" int ksim_preempt_spread(ksim_handle* h, const ksim_pod_set* ps, int32_t pod_index, int32_t priority,
                                   const ksim_pod_set* nps, int32_t n_groups, const int32_t* gnodes,
                                   const int32_t* first, const int32_t* count, ksim_preempt_out* out) {
  return preempt_run(h, ps, pod_index, priority, {nps, n_groups, gnodes, first, count}, out, PreemptEntry::spread);
}

// ---- the batched dry run --------------------------------------------------------
extern "C" int32_t ksim_preempt_many_rows(int32_t n_nodes, int32_t n_bound) {
  return preempt_many_rows(n_nodes, n_bound);
}
extern "C" int32_t ksim_preempt_many_dom_rows(int32_t n_nodes, int32_t n_bound, int32_t n_values) {
  return preempt_many_dom_rows(n_nodes, n_bound, n_values);
}

// The slabs of one launch group of `rows` rows (kept with the bound table),
// and for `dom_rows` of them the PreFilter states of domain rows.
static int many_slabs(ksim_handle* h, int32_t rows, int32_t dom_rows) {
  int rc;
  if (rows > h->bound.many.rows) {              // (every call ends synchronized: nothing reads them)
    h->bound.many.bufs.clear();
    h->bound.many.rows = 0;
    if ((rc = h->bound.many.bufs.alloc(h, h->bound.many.res, sizeof(PreemptNode) * (size_t)rows * std::max(h->dc.n, 1))) ||
        (rc = h->bound.many.bufs.alloc(h, h->bound.many.vflag, (size_t)rows * std::max(h->bound.n, 1))))
      return rc;
    h->bound.many.rows = rows;
  }
  if (dom_rows > h->bound.many.dom_rows) {
    h->bound.many.dom_bufs.clear();
    h->bound.many.dom_rows = 0;
    if ((rc = h->bound.many.dom_bufs.alloc(h, h->bound.many.dom, 8 * (size_t)dom_rows * KSIM_MAX_USES * h->dc.vmax)) ||
        (rc = h->bound.many.dom_bufs.alloc(h, h->bound.many.heads, sizeof(PreemptDomHead) * (size_t)dom_rows)))
      return rc;
    h->bound.many.dom_rows = dom_rows;
  }
  return KSIM_OK;
}

// Every row is ksim_preempt_full's dry run without nominated groups, against
// the same snapshot: a dry run changes nothing on the device, so the rows are
// independent.  The rows run in launch groups, one blockIdx.y each, every group
// uniform in its form:
//   0  FreeForm / PortsForm   Fit, host ports (uses no Filter reads beside them)
//   1  VolumeForm             counted volumes
//   2  SpreadForm             required pod (anti-)affinity, DoNotSchedule spread
//   3  FullForm               ... beside counted volumes
// A row of form 2 or 3 reads domain tables.  With `domains` (ksim_preempt_many_dom)
// it gets a PreFilter state of its own for its group; without (ksim_preempt_many)
// it runs the single-pod launches on the handle's tables after the groups.
// Everything is validated before anything runs.  fn: the entry point, as the
// error texts name it.
static int preempt_many_run(ksim_handle* h, const ksim_pod_set* ps, int32_t n, const int32_t* pod_index,
                            const int32_t* priority, ksim_preempt_out* outs, bool domains, const std::string& fn) {
  if (!h) return KSIM_E_INVALID;
  if (n < 0) return set_err(h, KSIM_E_INVALID, fn + ": negative row count");
  if (n == 0) return KSIM_OK;
  if (!ps || !pod_index || !priority || !outs) return set_err(h, KSIM_E_INVALID, fn + ": null argument");
  int rc = ensure_ready(h);
  if (rc) return rc;
  const NominatedGroups none{nullptr, 0, nullptr, nullptr, nullptr};
  std::vector<PreemptPlan> plans((size_t)n);
  for (int32_t i = 0; i < n; i++)
    if ((rc = preempt_check_args(h, ps, pod_index[i], none, &outs[i], PreemptEntry::full)) ||
        (rc = preempt_plan(h, ps, pod_index[i], priority[i], PreemptEntry::full, plans[i]))) {
      h->err = fn + " row " + std::to_string(i) + ": " + h->err;
      return rc;
    }
  HIPCHK(h, hipSetDevice(h->device));
  auto form_of = [](const PreemptPlan& q) {    // launch_preempt's choice of form
    const bool vol = q.vol.voff != nullptr;
    return q.reads_domains() ? (vol && q.vol.uses ? 3 : 2) : (vol ? 1 : 0);
  };
  // the rows of the launch groups, by form, each in the caller's order
  std::vector<int32_t> brow, bidx, bform;      // table position -> caller's row, its pod, its form
  for (int form = 0; form < (domains ? 4 : 2); form++)
    for (int32_t i = 0; i < n; i++)
      if (form_of(plans[i]) == form) {
        brow.push_back(i);
        bidx.push_back(pod_index[i]);
        bform.push_back(form);
      }
  const int32_t N = h->dc.n, nb = (int32_t)brow.size();
  std::vector<uint8_t> single((size_t)n, 1);
  if (nb > 0) {
    std::vector<DevPods> Ps;
    char *thost = nullptr, *tdev = nullptr;
    const size_t row_bytes = (sizeof(PreemptRow) * (size_t)nb + 63) / 64 * 64;   // then the domain rows' records
    if ((rc = upload_many(h, ps, bidx.data(), nb, row_bytes + sizeof(PreemptDomRow) * (size_t)nb, Ps, &thost, &tdev)))
      return rc;
    const int32_t R = preempt_many_rows(N, h->bound.n), RD = preempt_many_dom_rows(N, h->bound.n, h->dc.vmax);
    // a group ends with its form or at its form's row count
    std::vector<int32_t> gfirst((size_t)nb);    // table position -> its group's first position
    int32_t most = 0, most_dom = 0, n_dom = 0;
    for (int32_t k = 0, g0 = 0; k < nb; k++) {
      const bool dom = bform[k] >= 2;
      if (bform[k] != bform[g0] || k - g0 == (dom ? RD : R)) g0 = k;
      gfirst[k] = g0;
      most = std::max(most, k - g0 + 1);
      if (dom) most_dom = std::max(most_dom, k - g0 + 1), n_dom++;
    }
    if ((rc = many_slabs(h, most, most_dom))) return rc;
    // the result buffer: the pick records, then every row's victims list (no longer than a node's rows)
    std::vector<int32_t> vat((size_t)nb + 1, 0), dcap((size_t)nb);
    for (int32_t k = 0; k < nb; k++) {
      const ksim_preempt_out& o = outs[brow[k]];
      dcap[k] = o.victims && o.victims_cap > 0 ? std::min(o.victims_cap, h->bound.maxrow) : 0;
      vat[(size_t)k + 1] = vat[k] + dcap[k];
    }
    const size_t words = (size_t)kPickWords * nb + (size_t)vat[nb];
    if ((rc = h->many_out.reserve(h, 4 * words, Idle::kSync)) || (rc = h->many_host.reserve(h, 4 * words, Idle::kSync)))
      return rc;
    int32_t* dout = (int32_t*)h->many_out.p;
    const size_t dom_words = (size_t)KSIM_MAX_USES * h->dc.vmax;   // of one row's tables
    std::vector<PreemptRow> table((size_t)nb);
    std::vector<PreemptDomRow> dtable((size_t)nb);
    for (int32_t k = 0; k < nb; k++) {
      const int32_t at = k - gfirst[k];        // the row's place in its group: its slabs
      const PreemptPlan& q = plans[brow[k]];
      PreemptRow& r = table[k];
      r.P = Ps[k];
      r.vm = q.vol;
      r.res = h->bound.many.res + (size_t)at * N;
      r.vflag = h->bound.many.vflag + (size_t)at * std::max(h->bound.n, 1);
      r.victims = dout + (size_t)kPickWords * nb + vat[k];
      r.cap = dcap[k];
      r.prio = q.prio;
      r.ports = q.ports;
      r.vb = q.vb, r.vz = q.vz;
      PreemptDomRow& d = dtable[k];
      d = PreemptDomRow{};
      if (bform[k] >= 2) {
        d.dom = h->bound.many.dom + (size_t)at * dom_words;
        d.head = h->bound.many.heads + at;
        d.aff = q.aff, d.anti = q.anti, d.exist = q.exist, d.hard = q.hard;
      }
    }
    std::memcpy(thost, table.data(), sizeof(PreemptRow) * (size_t)nb);
    std::memcpy(thost + row_bytes, dtable.data(), sizeof(PreemptDomRow) * (size_t)nb);
    if ((rc = upload_many_commit(h))) return rc;
    const LaunchArgs a = make_args(h, DevPods{}, nullptr);
    DevPreempt pre = h->bound.d;
    pre.res = nullptr, pre.vflag = nullptr, pre.pick = nullptr, pre.nslot = nullptr;   // per row; no groups
    pre.afftot = nullptr;                      // (a domain row's is in its head)
    for (int32_t g0 = 0; g0 < nb;) {           // no host synchronization between the groups
      int32_t g1 = g0 + 1;
      while (g1 < nb && gfirst[g1] == g0) g1++;
      const int form = bform[g0];
      const PreemptMany g{(const PreemptRow*)tdev + g0, g1 - g0, form == 1, h->bound.many.res, dout + (size_t)kPickWords * g0,
                          h->bound.dindex, h->bp.rank_lo, h->bp.rank_hi};
      if (form >= 2) {
        bool spread = false;
        for (int32_t k = g0; k < g1; k++) spread |= plans[brow[k]].hard != 0;
        const PreemptManyDom d{(const PreemptDomRow*)(tdev + row_bytes) + g0, form == 3, spread};
        launch_preempt_many_dom(a, pre, plans[brow[g0]], g, d, h->stream);
      } else {
        launch_preempt_many(a, pre, plans[brow[g0]], g, h->stream);
      }
      HIPCHK(h, hipGetLastError());
      g0 = g1;
    }
    const int32_t* hout = (const int32_t*)h->many_host.p;
    HIPCHK(h, hipMemcpyAsync(h->many_host.p, dout, 4 * words, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int32_t k = 0; k < nb; k++) {
      const int32_t* pick = hout + (size_t)kPickWords * k;
      ksim_preempt_out& o = outs[brow[k]];
      o.nominated = pick[0];
      o.n_victims = pick[1];
      o.n_potential = pick[2];
      o.n_candidates = pick[3];
      o.n_pdb_violations = pick[4];
      if (pick[0] >= 0 && dcap[k] > 0)
        std::memcpy(o.victims, hout + (size_t)kPickWords * nb + vat[k],
                    4 * (size_t)std::min(pick[1], dcap[k]));
      single[brow[k]] = 0;
    }
    h->many_rows += nb - n_dom;
    h->many_dom_answered += n_dom;
  }
  for (int32_t i = 0; i < n && !domains; i++) {   // the rows that read domain tables, after the groups
    if (!single[i]) continue;
    if ((rc = preempt_run(h, ps, pod_index[i], priority[i], none, &outs[i], PreemptEntry::full))) return rc;
    h->many_single++;
  }
  return KSIM_OK;
}

extern "C" int ksim_preempt_many(ksim_handle* h, const ksim_pod_set* ps, int32_t n, const int32_t* pod_index,
                                 const int32_t* priority, ksim_preempt_out* outs) {
  return preempt_many_run(h, ps, n, pod_index, priority, outs, false, "ksim_preempt_many");
}

extern "C" int ksim_preempt_many_dom(ksim_handle* h, const ksim_pod_set* ps, int32_t n, const int32_t* pod_index,
                                     const int32_t* priority, ksim_preempt_out* outs) {
  return preempt_many_run(h, ps, n, pod_index, priority, outs, true, "ksim_preempt_many_dom");
}

// ---- committed preemption ---------------------------------------------------------
// The table's second buffer set and the scan's scratch, allocated at the first
// commit after ksim_set_bound_pods (a list's second buffers: after its setter)
// and kept until the table or the list goes.
static int commit_buffers(ksim_handle* h) {
  int rc;
  DevCommit& a = h->bound.alt;
  const size_t n = (size_t)std::max(h->bound.n, 1), N = (size_t)h->dc.n;
  if (!a.pos &&
      ((rc = h->bound.bufs.alloc(h, a.off2, 4 * (N + 1))) || (rc = h->bound.bufs.alloc(h, a.prio2, 4 * n)) ||
       (rc = h->bound.bufs.alloc(h, a.index2, 4 * n)) || (rc = h->bound.bufs.alloc(h, a.start2, 8 * n)) ||
       (rc = h->bound.bufs.alloc(h, a.req2, 8 * n * KSIM_PREEMPT_REQ)) ||
       (rc = h->bound.bufs.alloc(h, a.dead, n + 1)) || (rc = h->bound.bufs.alloc(h, a.before, 4 * (n + 1))) ||
       (rc = h->bound.bufs.alloc(h, a.tile, sizeof(CommitSum) * (size_t)commit_tiles(h->bound.n))) ||
       (rc = h->bound.bufs.alloc(h, a.pos, 4 * n))))   // pos last: set once the rest is there
    return rc;
  const size_t offs = 4 * ((size_t)h->bound.live + 1);
  if (h->bound.d.aoff && !a.aoff2 &&
      ((rc = h->bound.add.bufs.alloc(h, a.adds2, sizeof(ksim_class_add) * h->bound.add.ents)) ||
       (rc = h->bound.add.bufs.alloc(h, a.aoff2, offs))))
    return rc;
  if (h->bound.d.poff && !a.poff2 && ((rc = h->bound.pdb.bufs.alloc(h, a.pids2, 4 * h->bound.pdb.ents)) ||
                                  (rc = h->bound.pdb.bufs.alloc(h, a.poff2, offs))))
    return rc;
  if (h->bound.voff && !a.voff2 && ((rc = h->bound.vol.bufs.alloc(h, a.vols2, sizeof(VolHold) * h->bound.vol.ents)) ||
                                  (rc = h->bound.vol.bufs.alloc(h, a.voff2, offs))))
    return rc;
  return KSIM_OK;
}

// Bound-table rows rows[0 .. n) are evicted on the device: the snapshot as
// ksim_forget of pods[pod_index[i]] on each row's node leaves it, and the
// table, with the lists set on its rows, compacted to the rows left (their
// order and their numbers kept).  Everything is validated first; the host does
// O(n) work, the device passes are over the table (launch_preempt_commit), and
// the call ends with its one synchronization.
extern "C" int ksim_preempt_commit(ksim_handle* h, const ksim_pod_set* ps, int32_t n, const int32_t* rows,
                                   const int32_t* pod_index) {
  if (!h) return KSIM_E_INVALID;
  if (n < 0) return set_err(h, KSIM_E_INVALID, "ksim_preempt_commit: negative row count");
  if (n == 0) return KSIM_OK;
  if (!ps || !ps->pods || !rows || !pod_index) return set_err(h, KSIM_E_INVALID, "ksim_preempt_commit: null argument");
  int rc = ensure_ready(h);
  if (rc) return rc;
  if (is_sharded(h) || h->replicated)
    return set_err(h, KSIM_E_UNSUPPORTED, "ksim_preempt_commit: preemption runs on unsharded handles");
  if (!h->bound.d.off) return set_err(h, KSIM_E_INVALID, "ksim_preempt_commit: ksim_set_bound_pods first");
  // pre_dead[row] = 2 while this call names the row; the guard takes the marks back unless the call ran
  int32_t marked = 0;
  bool ran = false;
  struct Marks {
    ksim_handle* h;
    const int32_t* rows;
    const int32_t& marked;
    const bool& ran;
    ~Marks() {
      for (int32_t i = 0; i < marked; i++) h->bound.dead[rows[i]] = ran ? 1 : 0;
    }
  } marks{h, rows, marked, ran};
  for (int32_t i = 0; i < n; i++) {
    const std::string at = "ksim_preempt_commit entry " + std::to_string(i) + ": ";
    const int32_t r = rows[i], j = pod_index[i];
    if (r < 0 || r >= h->bound.n) return set_err(h, KSIM_E_INVALID, at + "row outside the bound-pod table");
    if (h->bound.dead[r] == 1) return set_err(h, KSIM_E_INVALID, at + "row already evicted");
    if (h->bound.dead[r] == 2) return set_err(h, KSIM_E_INVALID, at + "row named twice");
    if (j < 0 || j >= ps->n_pods) return set_err(h, KSIM_E_INVALID, at + "pod index outside the pod set");
    if ((rc = validate_pod(h, ps, j))) {
      h->err = at + h->err;
      return rc;
    }
    const ksim_pod& p = ps->pods[j];
    const int64_t* q = h->bound.row_req.data() + (size_t)r * KSIM_PREEMPT_REQ;
    bool same = p.req_cpu == q[0] && p.req_mem == q[1] && p.req_eph == q[2];
    for (int c = 0; c < KSIM_MAX_SCALAR; c++) same = same && p.scalar_req[c] == q[3 + c];
    if (!same) return set_err(h, KSIM_E_INVALID, at + "the pod's requests differ from the row's");
    h->bound.dead[r] = 2;
    marked = i + 1;
  }
  HIPCHK(h, hipSetDevice(h->device));
  if ((rc = commit_buffers(h))) return rc;
  std::vector<DevPods> Ps;
  char *thost = nullptr, *tdev = nullptr;
  if ((rc = upload_many(h, ps, pod_index, n, sizeof(CommitRec) * (size_t)n, Ps, &thost, &tdev))) return rc;
  CommitRec* recs = (CommitRec*)thost;
  for (int32_t i = 0; i < n; i++) recs[i] = CommitRec{Ps[i], rows[i], h->bound.row_node[rows[i]]};
  if ((rc = upload_many_commit(h))) return rc;
  DevPreempt& t = h->bound.d;
  DevCommit& a = h->bound.alt;
  DevCommit m = a;                               // the second set and the scratch; then the table as it is
  m.n = h->bound.live;
  m.n_nodes = h->dc.n;
  m.off = t.off, m.prio = t.prio, m.index = h->bound.dindex, m.start = t.start, m.req = t.req;
  m.aoff = t.aoff, m.adds = t.adds;
  m.poff = t.poff, m.pids = t.pids;
  m.voff = h->bound.voff, m.vols = h->bound.vols;
  launch_preempt_commit(h->dc, m, (const CommitRec*)tdev, n, h->stream);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));    // the staging is the next call's to write
  // the sets swap: the survivors' is the table now, the old one the next commit's target
  a.off2 = const_cast<int32_t*>(m.off), a.prio2 = const_cast<int32_t*>(m.prio);
  a.index2 = const_cast<int32_t*>(m.index), a.start2 = const_cast<int64_t*>(m.start);
  a.req2 = const_cast<int64_t*>(m.req);
  t.off = m.off2, t.prio = m.prio2, h->bound.dindex = m.index2, t.start = m.start2, t.req = m.req2;
  if (m.aoff) {
    a.aoff2 = const_cast<int32_t*>(m.aoff), a.adds2 = const_cast<ksim_class_add*>(m.adds);
    t.aoff = m.aoff2, t.adds = m.adds2;
  }
  if (m.poff) {
    a.poff2 = const_cast<int32_t*>(m.poff), a.pids2 = const_cast<int32_t*>(m.pids);
    t.poff = m.poff2, t.pids = m.pids2;
  }
  if (m.voff) {
    a.voff2 = const_cast<int32_t*>(m.voff), a.vols2 = const_cast<VolHold*>(m.vols);
    h->bound.voff = m.voff2, h->bound.vols = m.vols2;
  }
  h->bound.live -= n;
  h->bound.index_stale = true;
  ran = true;
  return KSIM_OK;
}

// ---- selector / affinity-term matching (ksim_match.hip) ------
extern "C" int ksim_match_terms(ksim_handle* h, const ksim_match_problem* mp, uint32_t* match_bits, int32_t* counts) {
  if (const int prc = flush_pend_bind(h)) return prc;   // a queued Reserve lands first
  if (!h || !mp || !match_bits) return set_err(h, KSIM_E_INVALID, "null argument");
  const ksim_match_problem& q = *mp;
  if (q.n_sigs < 0 || q.n_feat < 0 || q.n_reqs < 0 || q.n_matchers < 0 || q.n_pods < 0 || q.n_nodes < 0 ||
      q.n_classes < 0)
    return set_err(h, KSIM_E_INVALID, "negative size");
  if (q.n_reqs > kMatchMaxReqs || q.n_feat > kMatchMaxFeat)
    return set_err(h, KSIM_E_UNSUPPORTED, "match problem exceeds 4096 requirements or 65536 features");
  if (q.n_classes > 0 && !counts) return set_err(h, KSIM_E_INVALID, "counts buffer missing");
  if (!q.sig_feat_off || !q.req_feat_off || (!q.req_neg && q.n_reqs > 0) || !q.m_req_off)
    return set_err(h, KSIM_E_INVALID, "null CSR");
  // host validation: every index the kernels follow is in range
  auto csr_ok = [](const int32_t* off, int32_t rows, const int32_t* v, int32_t bound) {
    if (off[0] != 0) return false;
    for (int32_t i = 0; i < rows; i++)
      if (off[i + 1] < off[i]) return false;
    if (off[rows] > 0 && !v) return false;
    for (int32_t j = 0; j < off[rows]; j++)
      if (v[j] < 0 || v[j] >= bound) return false;
    return true;
  };
  if (!csr_ok(q.sig_feat_off, q.n_sigs, q.sig_feat, q.n_feat) ||
      !csr_ok(q.req_feat_off, q.n_reqs, q.req_feat, q.n_feat) ||
      !csr_ok(q.m_req_off, q.n_matchers, q.m_req, q.n_reqs))
    return set_err(h, KSIM_E_INVALID, "feature / requirement index out of range");
  if (q.n_classes > 0) {
    if (!q.class_matcher) return set_err(h, KSIM_E_INVALID, "class_matcher missing");
    for (int32_t c = 0; c < q.n_classes; c++)
      if (q.class_matcher[c] < 0 || q.class_matcher[c] >= q.n_matchers)
        return set_err(h, KSIM_E_INVALID, "class matcher out of range");
    if (q.n_pods > 0 && (!q.pod_sig || !q.pod_node)) return set_err(h, KSIM_E_INVALID, "bound pod arrays missing");
    for (int32_t p = 0; p < q.n_pods; p++)
      if (q.pod_sig[p] < 0 || q.pod_sig[p] >= q.n_sigs || q.pod_node[p] < 0 || q.pod_node[p] >= q.n_nodes)
        return set_err(h, KSIM_E_INVALID, "bound pod signature / node out of range");
  }
  if (q.n_sigs == 0) {                         // no signature: no bound pod either (pod_sig < n_sigs)
    if (q.n_classes > 0 && q.n_nodes > 0) std::memset(counts, 0, (size_t)q.n_classes * q.n_nodes * 4);
    return KSIM_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  DevMatch m{};
  m.s = q.n_sigs;
  m.sp = (q.n_sigs + 15) / 16 * 16;
  m.fp = std::max(64, (q.n_feat + 63) / 64 * 64);
  m.r = q.n_reqs;
  m.rp = std::max(16, (q.n_reqs + 15) / 16 * 16);
  m.m = q.n_matchers;
  m.w = (q.n_matchers + 31) / 32;
  m.c = q.n_classes;
  m.cw = (q.n_classes + 31) / 32;
  m.p = q.n_classes > 0 ? q.n_pods : 0;
  m.n = q.n_nodes;
  DevPool bufs;                                // this call's: freed on every way out
  int rc;
  std::vector<uint8_t> neg((size_t)m.rp, 0);
  std::copy(q.req_neg, q.req_neg + q.n_reqs, neg.begin());
  if ((rc = bufs.alloc(h, m.a, (size_t)m.sp * m.fp)) || (rc = bufs.alloc(h, m.bt, (size_t)m.rp * m.fp)) ||
      (rc = bufs.alloc(h, m.neg, neg.size(), neg.data())))
    return rc;
  auto put = [&](const int32_t* src, int64_t n, const int32_t*& dst) {
    return bufs.alloc(h, dst, (size_t)std::max<int64_t>(n, 0) * 4, src);
  };
  if ((rc = put(q.sig_feat_off, q.n_sigs + 1, m.sig_off)) || (rc = put(q.sig_feat, q.sig_feat_off[q.n_sigs], m.sig_feat)) ||
      (rc = put(q.req_feat_off, q.n_reqs + 1, m.req_off)) || (rc = put(q.req_feat, q.req_feat_off[q.n_reqs], m.req_feat)) ||
      (rc = put(q.m_req_off, q.n_matchers + 1, m.m_off)) || (rc = put(q.m_req, q.m_req_off[q.n_matchers], m.m_req)))
    return rc;
  if ((rc = bufs.alloc(h, m.bits, (size_t)m.s * std::max(m.w, 1) * 4))) return rc;
  if (m.c > 0) {
    if ((rc = put(q.class_matcher, m.c, m.cls_matcher)) || (rc = put(q.pod_sig, m.p, m.pod_sig)) ||
        (rc = put(q.pod_node, m.p, m.pod_node)) || (rc = bufs.alloc(h, m.cls_bits, (size_t)m.s * m.cw * 4)) ||
        (rc = bufs.alloc(h, m.cnt, (size_t)m.c * std::max(m.n, 1) * 4)))
      return rc;
  }
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  launch_match(m, h->stream);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  if (m.w > 0)
    HIPCHK(h, hipMemcpyAsync(match_bits, m.bits, (size_t)m.s * m.w * 4, hipMemcpyDeviceToHost, h->stream));
  if (m.c > 0 && m.n > 0)
    HIPCHK(h, hipMemcpyAsync(counts, m.cnt, (size_t)m.c * m.n * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float ms = 0.f;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  h->match_ns = (int64_t)(ms * 1e6);
  return KSIM_OK;
}
