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
// suffix of the node's range.  A pod with required pod (anti-)affinity uses
// takes the domain form: the thread holds the node's TopoRow (the domain sum of
// the node's topology value, or the node's own count, per use), moves it the
// same way and re-runs interpodaffinity's Filter on it; a node that failed
// InterPodAffinity for an anti-affinity reason is a potential node too.  With
// PodDisruptionBudgets on the table (ksim_set_bound_pod_pdbs) the thread first
// splits the lower-priority pods as filterPodsWithPDBViolation does (the PDB
// form, kernels of their own) and reprieves the violating ones first.  A pod
// with DoNotSchedule spread uses (ksim_preempt_spread) takes the spread form:
// the domain form plus PodTopologySpread's Filter on the moved row, against
// min(the node's own domain, the minimum over the other present domains),
// which k_preempt_spread_mins takes once per dry run.  A pod with counted
// volumes (ksim_preempt_volumes) takes the volume form, k_preempt_nodes_vol:
// the ports form plus the node volume limit plugins on the node's attached
// count per family, moved with the rows' holdings (ksim_set_bound_pod_volumes);
// a node that failed one of those plugins is a potential node too.  A pod with
// counted volumes beside (anti-)affinity or spread uses (ksim_preempt_full)
// takes the full form, k_preempt_nodes_full: the spread form and the volume
// form in one thread; for a pod with volume groups k_preempt_static_veto then
// takes the nodes VolumeBinding or VolumeZone fails out of the candidates.  One
// block then keeps candidates in nodeTree order (upstream scans from a random
// offset; offset 0 here) until numCandidates were found and one of them has
// no PDB violation, and picks one by pickOneNodeForPreemption's criteria.
#include "ksim_device.h"
#include "ksim_internal.h"
#include "ksim_wave.h"

#include <type_traits>

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

// The volume form's per-thread state: the node's distinct family-f volumes
// (c.vol_attached, moved with every pod taken out or put back) and its limit,
// for the families the preemptor has a use of.  Indexed by unrolled constants
// only, so both stay in registers.
struct VolRow {
  int64_t att[KSIM_MAX_VOL_FAMILIES];
  int32_t lim[KSIM_MAX_VOL_FAMILIES];
};
struct NoVol {};                                         // the other forms' (empty) volume argument
// The full form's holder counts: the TopoRow's own entries (load_topo_row put a
// volume use's class count there), under the name the volume form reads.
struct RowHold {
  int64_t (&held)[KSIM_MAX_USES];
};
// The volume side's holder counts of a form: the row's in the full form (ROW),
// held[] in the volume form.
template <bool ROW>
__device__ __forceinline__ decltype(auto) vol_holder(PortHold& h, TopoRow& t) {
  if constexpr (ROW) return RowHold{t.x};
  else return (h);
}
// nodeports Filter on the holdings of the volume form: only the port uses
// conflict (a held volume class is no conflict)
__device__ __forceinline__ bool hold_conflict(const PortHold& h, uint32_t port_mask) {
  bool hit = false;
#pragma unroll
  for (int i = 0; i < KSIM_MAX_USES; i++)
    if (((port_mask >> i) & 1u) && h.held[i] > 0) hit = true;
  return hit;
}
// Pods of the node's suffix [j0, b) that are out of the trial state (bit 0 of
// their flag; row `skip` apart) and hold volume class `cls`: a direct count,
// quadratic in the node's victims like the PDB form's.
__device__ __forceinline__ int32_t vol_out_holders(const DevPreempt& pre, const PreemptVol& vm, int32_t j0, int32_t b,
                                                   int32_t skip, int32_t cls) {
  int32_t n = 0;
  for (int32_t k = j0; k < b; k++) {
    if (k == skip || !(pre.vflag[k] & 1)) continue;
    for (int32_t e = vm.voff[k]; e < vm.voff[k + 1]; e++) n += vm.vols[e].cls == cls;
  }
  return n;
}
// Entries [e0, e1) of `ents` that hold class `cls`
__device__ __forceinline__ int32_t vol_class_entries(const VolHold* __restrict__ ents, int32_t e0, int32_t e1,
                                                     int32_t cls) {
  int32_t n = 0;
  for (int32_t e = e0; e < e1; e++) n += ents[e].cls == cls;
  return n;
}
// The holders of volume class x on the node apart from row j, for a class the
// preemptor does not use: the device's count (every bound holder of the node,
// whatever its priority, row j among them) and the nominated group's, less the
// rows that are out.
struct VolOthers {
  const DevCluster& c;
  const DevPreempt& pre;
  const PreemptVol& vm;
  int32_t node, g, j0, b, j;
  __device__ __forceinline__ int32_t operator()(int32_t x, int32_t) const {
    const int32_t grp = g >= 0 ? vol_class_entries(vm.gvols, vm.gvoff[g], vm.gvoff[g + 1], x) : 0;
    return (int32_t)class_count(c, x, node) - 1 + grp - vol_out_holders(pre, vm, j0, b, j, x);
  }
};
// NodeInfo.AddPod / RemovePod on the node's attached volumes (volume_bind's
// rule on the thread's copy): the holdings [e0, e1) of one pod.  A classless
// holding moves its family's count by arg.  A class holding moves it by one
// when no other pod on the node holds the volume: for a class of the
// preemptor's that is held[i] (moved here too), for any other class
// others(cls, e) counts the other holders.  Families the preemptor has no use
// of are not read.
template <typename OTHERS, typename HOLD>
__device__ __forceinline__ void vol_add(VolRow& v, HOLD&& h, const int32_t (&cls)[KSIM_MAX_USES],
                                        const PreemptVol& vm, const VolHold* __restrict__ ents, int32_t e0,
                                        int32_t e1, int sign, OTHERS others) {
  for (int32_t e = e0; e < e1; e++) {
    const VolHold x = ents[e];
    if (!((vm.fams >> x.fam) & 1u)) continue;
    int64_t d = (int64_t)sign * x.arg;
    if (x.cls >= 0) {
      bool mine = false;
      int32_t rest = 0;                                  // the volume's other holders on the node
#pragma unroll
      for (int i = 0; i < KSIM_MAX_USES; i++)
        if (((vm.uses >> i) & 1u) && cls[i] == x.cls) {
          mine = true;
          rest = (int32_t)(sign < 0 ? h.held[i] - 1 : h.held[i]);
          h.held[i] += sign;
        }
      if (!mine) rest = others(x.cls, e);
      d = rest == 0 ? sign : 0;
    }
#pragma unroll
    for (int k = 0; k < KSIM_MAX_VOL_FAMILIES; k++)
      if (k == x.fam) v.att[k] += d;
  }
}
// nodevolumelimits Filter on the moved counts (volume_limit_fails' rule, 64-bit
// sums): per family of the preemptor's, new = its classless volumes (own[f])
// plus its class volumes no pod left on the node holds.  ufam: four bits per
// use, the family of volume use i.
template <typename HOLD>
__device__ __forceinline__ bool vol_fails(const VolRow& v, const HOLD& h, const int32_t (&cls)[KSIM_MAX_USES],
                                          const PreemptVol& vm, uint64_t ufam,
                                          const int64_t (&own)[KSIM_MAX_VOL_FAMILIES]) {
  bool bad = false;
#pragma unroll
  for (int k = 0; k < KSIM_MAX_VOL_FAMILIES; k++) {
    if (!((vm.fams >> k) & 1u)) continue;
    int64_t add = own[k];
#pragma unroll
    for (int i = 0; i < KSIM_MAX_USES; i++)
      if (((vm.uses >> i) & 1u) && cls[i] >= 0 && (int)((ufam >> (4 * i)) & 15u) == k) add += h.held[i] == 0;
    const bool csi = (vm.csi >> k) & 1u;
    if (v.lim[k] != 2147483647 && v.att[k] + add > (int64_t)v.lim[k] && (!csi || add > 0)) bad = true;
  }
  return bad;
}

// The preemptor's filter-read uses in the domain form (kernel argument, bit i =
// use i): its InterPodAffinity uses by role when the profile filters on them,
// and that filter's place in the profile.  All zero: no domain form.
struct PreemptDom {
  uint32_t aff, anti, exist;
  int32_t ipa_index;
};
// The spread form's argument (the other forms keep PreemptDom, and with it
// their kernel arguments): the preemptor's DoNotSchedule spread uses when the
// profile filters on PodTopologySpread, that filter's place, and per use
// {the minimum over the present domains, the value id of one arg-min, the
// minimum over the others} (k_preempt_spread_mins; [KSIM_MAX_USES][3]).
struct PreemptSpread : PreemptDom {
  uint32_t hard;
  int32_t pts_index;
  int64_t* smin;
};
// NodeInfo.AddPod / RemovePod and PreFilterExtensions.AddPod / RemovePod of one
// pod (or nominated group) on the node's row: sign x count of every add whose
// class a filter-read use reads.  A use whose key the node lacks (t.v[i] == 0)
// moves too, but no Filter reads its count (upstream leaves its maps alone).
// A DoNotSchedule spread use's entry carries the presence marks above its
// count (kDomMarkShift): the count of the pods the status pass summed never
// goes below zero, so adding to the whole entry leaves the marks alone; such a
// use moves only on a node that is eligible for it (its cls[i] is
// kNoPortClass elsewhere: podtopologyspread's updateWithPod).
__device__ __forceinline__ void topo_add(TopoRow& t, const int32_t (&cls)[KSIM_MAX_USES],
                                         const ksim_class_add* __restrict__ adds, int32_t e0, int32_t e1, int sign) {
  for (int32_t e = e0; e < e1; e++) {
    const ksim_class_add x = adds[e];
#pragma unroll
    for (int i = 0; i < KSIM_MAX_USES; i++)
      if (cls[i] == x.cls) t.x[i] += (int64_t)sign * x.count;
  }
}
// podtopologyspread Filter on the moved row -> 0 or KSIM_PTS_* (the first
// failing constraint's reason, as pts_filter).  Constraint i fails for skew
// when match + selfMatch - crit > maxSkew, crit = min(match, others_i) on a
// node that is eligible for it (its own domain is present and moves) and
// others_i elsewhere (nothing moved: the status pass's minimum).  With
// thr[i] = others_i - (selfMatch - maxSkew), fixed for the dry run, that is
// match > thr[i], or selfMatch > maxSkew on an eligible node (bit i of `over`:
// the own domain alone is too many).
__device__ __forceinline__ uint32_t spread_filter(uint32_t hard, uint32_t over, const int64_t (&thr)[KSIM_MAX_USES],
                                                  const TopoRow& t) {
  uint32_t why = 0;
#pragma unroll
  for (int i = 0; i < KSIM_MAX_USES; i++) {
    if (why != 0 || !((hard >> i) & 1u)) continue;
    const int64_t match = t.x[i] & kDomCountMask;                  // absent pair: 0
    if (t.v[i] == 0) why = KSIM_PTS_MISSING_LABEL;
    else if (((over >> i) & 1u) || match > thr[i]) why = KSIM_PTS_SKEW;
  }
  return why;
}
// spread_filter(...) != 0 without the order of the reasons: what a trial asks
__device__ __forceinline__ bool spread_fails(uint32_t hard, uint32_t over, const int64_t (&thr)[KSIM_MAX_USES],
                                             const TopoRow& t) {
  bool bad = (hard & over) != 0;
#pragma unroll
  for (int i = 0; i < KSIM_MAX_USES; i++)
    if ((hard >> i) & 1u) bad |= t.v[i] == 0 || (t.x[i] & kDomCountMask) > thr[i];
  return bad;
}
// len(state.affinityCounts) > 0 on the moved row: a matching pod outside the
// node's domains (outside: the use's cluster-wide total minus the node's domain
// sum, neither of which another node's dry run changes), or one left inside
__device__ __forceinline__ uint32_t affinity_flags(uint32_t aff, bool outside, const TopoRow& t) {
  bool any = outside;
#pragma unroll
  for (int i = 0; i < KSIM_MAX_USES; i++)
    if (((aff >> i) & 1u) && t.v[i] != 0 && t.x[i] > 0) any = true;
  return any ? kTopoAffinityNonEmpty : 0u;
}

// SelectVictimsOnNode of one potential node.  PORTS: the dry run re-runs
// NodePorts beside NodeResourcesFit (the preemptor has port uses and the
// profile filters on them); fit: the profile has NodeResourcesFit.
// DOM (the domain form): the dry run re-runs NodePorts and InterPodAffinity on
// the node's TopoRow.  The node failed at Fit, NodePorts or InterPodAffinity;
// the last is a potential node only for an anti-affinity reason, which the
// thread re-derives from the row (with the nominated group on it: pass 1).
// PDB (the PDB form): the table carries budgets (pre.poff / pids / pallowed).
// filterPodsWithPDBViolation walks the suffix most important first with a
// fresh copy of every budget and decrements each budget a pod matches; the pod
// violates when one of them went below zero, i.e. when the rows of [j0, j]
// that carry the budget outnumber its disruptionsAllowed.  That count is taken
// directly (quadratic in the node's victims, no per-thread array, no cap on
// the number of budgets).  The violating rows are reprieved first, then the
// others, so the victims list need not be sorted by priority: `high` is the
// first victim appended, `early` follows the true maximum priority.
// SPREAD (the spread form; implies DOM): the dry run also re-runs
// PodTopologySpread on the row.  In node n's dry run only n's pods move, so
// per constraint only the count of n's own domain moves and the critical path
// is min(own count, others_i): the minimum over the other present domains
// (dm.smin: the second minimum when n's value is the arg-min), fixed for the
// whole dry run and folded into thr[i].  A pod of n moves constraint i only when n is
// eligible for it (every hard constraint's key on n, and n passes i's node
// inclusion policies: what k_topo_prefilter counted); elsewhere the verdict
// is the status pass's.  A node that failed PodTopologySpread is a potential
// node only for the skew reason, re-derived from the row like
// InterPodAffinity's.
// VOL (the volume form; PORTS with it): the dry run also re-runs the node
// volume limit plugins of the profile.  The thread keeps the node's attached
// count per family of the preemptor's (VolRow) and, in held[], the node's count
// of each shared volume the preemptor mounts, beside its port classes (the ids
// are disjoint; a classless volume use keeps kNoPortClass).  Both move with
// the rows' holdings (vm.voff / vols); bit 0 of a row's flag says "out of the
// trial state" from the first removal on, which is what it says at the end.
// VOL with DOM and SPREAD (the full form): both sides at once.  Ports, affinity
// and spread counts move in the TopoRow by the class adds; VolRow moves by the
// holdings, and a shared volume's holder count is the row's own entry of the
// volume use (RowHold) instead of held[], which the full form does not keep.
template <bool PORTS, bool DOM = false, bool PDB = false, bool SPREAD = false, typename DM = PreemptDom,
          bool VOL = false, typename VM = NoVol>
__device__ __forceinline__ void select_victims(const DevCluster& c, const DevPods& P, const DevScratch& s,
                                               const ksim_pod& p, const PodPlan& plan, const ksim_topo_use* U,
                                               const DevPreempt& pre, int32_t node, int32_t prio, bool fit,
                                               uint32_t port_mask, const DM& dm, bool at_ipa, bool at_pts,
                                               PreemptNode& out, const VM& vm = VM{}) {
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
  TopoRow t;
  UseMasks mm{};                                        // the roles the dry run's filters read
  bool outside = false;
  VolRow vr;                                            // VOL: the families' moved counts and limits
  uint64_t ufam = 0;                                    // VOL: the family of each volume use, four bits each
  int64_t own[KSIM_MAX_VOL_FAMILIES];                   // VOL: per family, the preemptor's classless volumes
  uint32_t elig = 0, over = 0;                          // SPREAD: the hard uses this node's pods move; spread_filter
  int64_t thr[KSIM_MAX_USES];                           // SPREAD: per hard use, the count the row may reach
  if (DOM) {
    mm.port = port_mask;
    mm.aff = dm.aff;
    mm.anti = dm.anti;
    mm.exist = dm.exist;
    const uint32_t read = port_mask | dm.aff | dm.anti | dm.exist;
    load_topo_row(c, U, p.use_count, plan.m, s, P.ptab, node, t);
    if constexpr (SPREAD) {                             // updateWithPod's node tests, once per node
      bool all_hard = true;                             // nodeLabelsMatchSpreadConstraints
#pragma unroll
      for (int i = 0; i < KSIM_MAX_USES; i++)
        if (((dm.hard >> i) & 1u) && t.v[i] == 0) all_hard = false;
      if (all_hard) {                                   // matchNodeInclusionPolicies, as k_topo_prefilter
        const bool aff_ok = (plan.m.honor_aff & dm.hard) ? required_node_affinity_match(c, P, p, node) : true;
        const bool taint_ok = (plan.m.honor_taints & dm.hard) ? !node_has_untolerated_taint(c, p, node) : true;
        elig = dm.hard & ~(aff_ok ? 0u : plan.m.honor_aff) & ~(taint_ok ? 0u : plan.m.honor_taints);
      }
    }
#pragma unroll
    for (int i = 0; i < KSIM_MAX_USES; i++) {
      cls[i] = kNoPortClass;
      if ((read >> i) & 1u) cls[i] = load_use(U, i).cls;
      if (((dm.aff >> i) & 1u) && t.v[i] != 0 && pre.afftot[i] - t.x[i] > 0) outside = true;
      if constexpr (SPREAD) {
        thr[i] = 0;
        if ((dm.hard >> i) & 1u) {
          const int64_t* mn = dm.smin + 3 * i;          // {min1, the arg-min's value id, min2}
          const ksim_topo_use u = load_use(U, i);
          const bool mine = (elig >> i) & 1u;
          // others_i(n): the second minimum when n's own domain is the arg-min
          const int64_t oth = mine && (int64_t)t.v[i] == mn[1] ? mn[2] : mn[0];
          const int64_t lim = (int64_t)((plan.m.self_match >> i) & 1u) - (int64_t)u.arg;
          thr[i] = oth - lim;
          if (mine && lim > 0) over |= 1u << i;
          if (mine) cls[i] = u.cls;
        }
      }
    }
    if (g >= 0) topo_add(t, cls, pre.gadds, pre.goff[g], pre.goff[g + 1], 1);
    if constexpr (SPREAD) {
      if (at_pts && spread_filter(dm.hard, over, thr, t) == KSIM_PTS_MISSING_LABEL)
        return;                                         // the status pass's detail: UnschedulableAndUnresolvable
    }
    if (at_ipa) {                                       // the status pass's InterPodAffinity detail
      const uint32_t why = ipa_filter(mm, p, affinity_flags(dm.aff, outside, t), t);
      if (why != KSIM_IPA_ANTI_AFFINITY && why != KSIM_IPA_EXISTING_ANTI) return;   // UnschedulableAndUnresolvable
    }
    out.potential = 1;
  }
  decltype(auto) hv = vol_holder<VOL && DOM>(h, t);      // VOL: the shared volumes' holder counts
  if constexpr (VOL && DOM) {                           // the full form's volume side, as the volume form's below
    ufam = 0;
#pragma unroll
    for (int k = 0; k < KSIM_MAX_VOL_FAMILIES; k++) {
      own[k] = 0;
      vr.att[k] = 0;
      vr.lim[k] = 2147483647;
      if ((vm.fams >> k) & 1u) {
        vr.att[k] = c.vol_attached[(size_t)k * c.n + node];
        vr.lim[k] = c.vol_limit[(size_t)k * c.n + node];
      }
    }
#pragma unroll
    for (int i = 0; i < KSIM_MAX_USES; i++) {
      if (!((vm.uses >> i) & 1u)) continue;
      const ksim_topo_use u = load_use(U, i);            // the device copy: family in _pad
      ufam |= (uint64_t)(u._pad & 15) << (4 * i);
      if (u.cls >= 0) {
        cls[i] = u.cls;                                  // t.x[i]: the node's holders (load_topo_row); no add names it
      } else {
#pragma unroll
        for (int k = 0; k < KSIM_MAX_VOL_FAMILIES; k++)
          if (k == u._pad) own[k] += u.arg;
      }
    }
    if (g >= 0) {                                        // the group's volumes, each pod after the ones before it
      const int32_t g0 = vm.gvoff[g];
      vol_add(vr, hv, cls, vm, vm.gvols, g0, vm.gvoff[g + 1], 1, [&](int32_t x, int32_t e) {
        return class_count(c, x, node) + vol_class_entries(vm.gvols, g0, e, x);
      });
    }
    for (int32_t j = j0; j < b; j++) pre.vflag[j] = 0;   // nobody is out yet
  }
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
    if constexpr (VOL) {
      ufam = 0;
#pragma unroll
      for (int k = 0; k < KSIM_MAX_VOL_FAMILIES; k++) {
        own[k] = 0;
        vr.att[k] = 0;
        vr.lim[k] = 2147483647;
        if ((vm.fams >> k) & 1u) {
          vr.att[k] = c.vol_attached[(size_t)k * c.n + node];
          vr.lim[k] = c.vol_limit[(size_t)k * c.n + node];
        }
      }
#pragma unroll
      for (int i = 0; i < KSIM_MAX_USES; i++) {
        if (!((vm.uses >> i) & 1u)) continue;
        const ksim_topo_use u = load_use(U, i);          // the device copy: family in _pad
        ufam |= (uint64_t)(u._pad & 15) << (4 * i);
        if (u.cls >= 0) {
          cls[i] = u.cls;
          h.held[i] = (int32_t)class_count(c, u.cls, node);
        } else {
#pragma unroll
          for (int k = 0; k < KSIM_MAX_VOL_FAMILIES; k++)
            if (k == u._pad) own[k] += u.arg;
        }
      }
    }
    if (g >= 0 && (!VOL || port_mask)) hold_add(h, cls, pre.gadds, pre.goff[g], pre.goff[g + 1], 1);
    if constexpr (VOL) {
      if (g >= 0) {                                      // the group's volumes, each pod after the ones before it
        const int32_t g0 = vm.gvoff[g];
        vol_add(vr, hv, cls, vm, vm.gvols, g0, vm.gvoff[g + 1], 1, [&](int32_t x, int32_t e) {
          return class_count(c, x, node) + vol_class_entries(vm.gvols, g0, e, x);
        });
      }
      for (int32_t j = j0; j < b; j++) pre.vflag[j] = 0; // nobody is out yet
    }
  }
  for (int32_t j = j0; j < b; j++) {
    row_add_req(r, pre.req + (size_t)j * KSIM_PREEMPT_REQ, -1, c.n_scalar);
    if (PORTS && (!VOL || port_mask)) hold_add(h, cls, pre.adds, pre.aoff[j], pre.aoff[j + 1], -1);
    if constexpr (VOL) {
      vol_add(vr, hv, cls, vm, vm.vols, vm.voff[j], vm.voff[j + 1], -1, VolOthers{c, pre, vm, node, g, j0, b, j});
      pre.vflag[j] = 1;
    }
    if (DOM) topo_add(t, cls, pre.adds, pre.aoff[j], pre.aoff[j + 1], -1);
  }
  // the filters the dry run re-runs: 0 = the pod passes
  auto fails = [&]() -> bool {
    if ((!(PORTS || DOM) || fit) && fits_request(r, p, c.n_scalar, c.fit_ignore) != 0) return true;
    if constexpr (SPREAD) {
      if (spread_fails(dm.hard, over, thr, t)) return true;
    }
    if constexpr (VOL && DOM) {
      if (vol_fails(vr, hv, cls, vm, ufam, own)) return true;
    }
    if (DOM) return node_port_conflict(mm, t) || ipa_filter(mm, p, affinity_flags(dm.aff, outside, t), t) != 0;
    if constexpr (VOL) return hold_conflict(h, port_mask) || vol_fails(vr, hv, cls, vm, ufam, own);
    return PORTS && hold_conflict(h);
  };
  if (!fails()) {
    out.cand = 1;
    if (PDB) {                                          // filterPodsWithPDBViolation
      for (int32_t j = j0; j < b; j++) {
        bool viol = false;
        for (int32_t e = pre.poff[j]; e < pre.poff[j + 1]; e++) {
          const int32_t id = pre.pids[e];
          int32_t used = 0;                             // rows of [j0, j] in budget id (j itself among them)
          for (int32_t e2 = pre.poff[j0]; e2 < pre.poff[j + 1]; e2++) used += pre.pids[e2] == id;
          if (used > pre.pallowed[id]) viol = true;
        }
        pre.vflag[j] = (viol ? kPreemptViolating : 0) | (VOL ? 1 : 0);
      }
    }
    int32_t nv = 0, nviol = 0, high = 0, top = INT32_MIN;
    int64_t sum = 0, early = INT64_MAX;
    for (int pass = PDB ? 0 : 1; pass < 2; pass++) {     // the violating rows first, then the others
      for (int32_t j = j0; j < b; j++) {                 // reprievePod, most important first
        uint8_t mark = 0;
        if (PDB) {
          mark = pre.vflag[j] & kPreemptViolating;
          if ((mark != 0) != (pass == 0)) continue;
        }
        const int64_t* q = pre.req + (size_t)j * KSIM_PREEMPT_REQ;
        row_add_req(r, q, 1, c.n_scalar);
        if (PORTS && (!VOL || port_mask)) hold_add(h, cls, pre.adds, pre.aoff[j], pre.aoff[j + 1], 1);
        if (DOM) topo_add(t, cls, pre.adds, pre.aoff[j], pre.aoff[j + 1], 1);
        if constexpr (VOL)
          vol_add(vr, hv, cls, vm, vm.vols, vm.voff[j], vm.voff[j + 1], 1, VolOthers{c, pre, vm, node, g, j0, b, j});
        const bool victim = fails();
        pre.vflag[j] = (uint8_t)victim | mark;
        if (victim) {
          row_add_req(r, q, -1, c.n_scalar);
          if (PORTS && (!VOL || port_mask)) hold_add(h, cls, pre.adds, pre.aoff[j], pre.aoff[j + 1], -1);
          if (DOM) topo_add(t, cls, pre.adds, pre.aoff[j], pre.aoff[j + 1], -1);
          if constexpr (VOL)
            vol_add(vr, hv, cls, vm, vm.vols, vm.voff[j], vm.voff[j + 1], -1, VolOthers{c, pre, vm, node, g, j0, b, j});
          if (nv == 0) high = pre.prio[j];
          sum += (int64_t)pre.prio[j] + ((int64_t)INT32_MAX + 1);
          if (PDB) {                                     // GetEarliestPodStartTime on an unsorted list
            if (pre.prio[j] > top || nv == 0) {
              top = pre.prio[j];
              early = pre.start[j];
            } else if (pre.prio[j] == top && pre.start[j] < early) {
              early = pre.start[j];
            }
            if (mark) nviol++;
          } else if (pre.prio[j] == high && pre.start[j] < early) {
            early = pre.start[j];                        // sorted list: the first victim is the highest
          }
          nv++;
        }
      }
    }
    out.nv = nv;
    if (PDB) out.cand |= nviol << 1;
    out.high = nv ? high : INT32_MIN;
    out.sum = sum;
    out.early = early;
  } else {
    for (int32_t j = j0; j < b; j++) pre.vflag[j] = 0;
  }
}

// Per node: SelectVictimsOnNode.  res[node] = {potential, candidate (with the
// PDB violations among the victims above bit 0), victims, the first victim's
// priority, sum of (priority + 2^31), earliest start among the
// highest-priority victims}; vflag marks the victims (bit 0) and, in the PDB
// form, the violating rows (bit 1), in CSR order.  A potential
// node failed NodeResourcesFit or, for a preemptor with port uses (port_mask),
// NodePorts or, for one with required pod (anti-)affinity uses (dm),
// InterPodAffinity with an anti-affinity detail: the filters that return
// Unschedulable and that the dry run re-runs.  DOM: the domain form, a kernel
// of its own, so a preemptor without such uses runs the code (and keeps the
// registers) it had before that form existed.  PDB: the PDB form, likewise
// kernels of their own, launched only when the table carries budgets.
// SPREAD: the spread form (ksim_preempt_spread for a preemptor with
// DoNotSchedule spread uses; DOM with it), kernels of their own again: a node
// that failed PodTopologySpread for the skew reason is a potential node too.
template <bool DOM, bool PDB, bool SPREAD = false>
__global__ __launch_bounds__(256) void k_preempt_nodes(DevCluster c, DevPods P, const DevState* __restrict__ st,
                                                       DevScratch s, DevPreempt pre, int32_t fit_index,
                                                       int32_t prio, int32_t port_index, uint32_t port_mask,
                                                       std::conditional_t<SPREAD, PreemptSpread, PreemptDom> dm) {
  const int32_t node = blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= c.n) return;
  PreemptNode out{};
  out.cand = 0;
  const uint8_t f = s.fail[node];
  const ksim_pod& p = P.pods[st->cursor];
  const ksim_topo_use* U = P.uses + p.use_first;
  if constexpr (SPREAD) {
    const bool at_ipa = (dm.aff | dm.anti | dm.exist) != 0 && f == (uint8_t)dm.ipa_index;
    const bool at_pts = f == (uint8_t)dm.pts_index;
    if ((fit_index >= 0 && f == (uint8_t)fit_index) || (port_mask && f == (uint8_t)port_index) || at_ipa || at_pts)
      select_victims<false, true, PDB, true>(c, P, s, p, P.plans[st->cursor], U, pre, node, prio, fit_index >= 0,
                                             port_mask, dm, at_ipa, at_pts, out);
  } else if (DOM) {
    const bool at_ipa = f == (uint8_t)dm.ipa_index;
    if ((fit_index >= 0 && f == (uint8_t)fit_index) || (port_mask && f == (uint8_t)port_index) || at_ipa)
      select_victims<false, true, PDB>(c, P, s, p, P.plans[st->cursor], U, pre, node, prio, fit_index >= 0, port_mask, dm,
                                  at_ipa, false, out);
  } else {
    const bool potential = (fit_index >= 0 && f == (uint8_t)fit_index) || (port_mask && f == (uint8_t)port_index);
    out.potential = potential;
    if (potential) {
      if (port_mask)                                   // kernel argument: one uniform branch
        select_victims<true, false, PDB>(c, P, s, p, P.plans[st->cursor], U, pre, node, prio, fit_index >= 0, port_mask, dm,
                             false, false, out);
      else
        select_victims<false, false, PDB>(c, P, s, p, P.plans[st->cursor], U, pre, node, prio, true, 0u, dm, false, false,
                                          out);
    }
  }
  pre.res[node] = out;
}

// k_preempt_nodes for a preemptor with KSIM_USE_VOLUME uses (ksim_preempt_volumes):
// the volume form, kernels of their own with an argument of their own, so the
// forms above keep theirs.  The four limit plugins return Unschedulable, so a
// node whose first failing filter is one of them (vm.at: their places in the
// profile) is a potential node beside Fit's and NodePorts'.
template <bool PDB>
__global__ __launch_bounds__(256) void k_preempt_nodes_vol(DevCluster c, DevPods P, const DevState* __restrict__ st,
                                                           DevScratch s, DevPreempt pre, int32_t fit_index,
                                                           int32_t prio, int32_t port_index, uint32_t port_mask,
                                                           PreemptVol vm) {
  const int32_t node = blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= c.n) return;
  PreemptNode out{};
  out.cand = 0;
  const uint32_t f = s.fail[node];
  const ksim_pod& p = P.pods[st->cursor];
  bool potential = (fit_index >= 0 && f == (uint32_t)fit_index) || (port_mask && f == (uint32_t)port_index);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t at = (vm.at >> (8 * k)) & 255u;      // 0xff: absent (KSIM_PASSED is no plugin's place)
    if (at != 255u && f == at) potential = true;
  }
  out.potential = potential;
  if (potential)
    select_victims<true, false, PDB, false, PreemptDom, true, PreemptVol>(
        c, P, s, p, P.plans[st->cursor], P.uses + p.use_first, pre, node, prio, fit_index >= 0, port_mask, PreemptDom{},
        false, false, out, vm);
  pre.res[node] = out;
}

// k_preempt_nodes for a preemptor with KSIM_USE_VOLUME uses beside required pod
// (anti-)affinity or DoNotSchedule spread uses (ksim_preempt_full): the full
// form, the spread form and the volume form in one thread, kernels of their
// own again with both arguments.  The thread keeps one TopoRow, moved by
// topo_add over the rows' class adds (ports, affinity and spread counts), and
// VolRow, moved by vol_add over the rows' holdings; a shared volume's holder
// count lives in the row's own entry (no add names a volume class, so only
// vol_add moves it).  ds.hard may be empty (volumes beside affinity alone):
// then no use is a spread use and PodTopologySpread's place is not read.
template <bool PDB>
__global__ __launch_bounds__(256) void k_preempt_nodes_full(DevCluster c, DevPods P, const DevState* __restrict__ st,
                                                            DevScratch s, DevPreempt pre, int32_t fit_index,
                                                            int32_t prio, int32_t port_index, uint32_t port_mask,
                                                            PreemptSpread ds, PreemptVol vm) {
  const int32_t node = blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= c.n) return;
  PreemptNode out{};
  out.cand = 0;
  const uint32_t f = s.fail[node];
  const ksim_pod& p = P.pods[st->cursor];
  const bool at_ipa = (ds.aff | ds.anti | ds.exist) != 0 && f == (uint32_t)ds.ipa_index;
  const bool at_pts = ds.hard != 0 && f == (uint32_t)ds.pts_index;
  bool enter = (fit_index >= 0 && f == (uint32_t)fit_index) || (port_mask && f == (uint32_t)port_index) || at_ipa ||
               at_pts;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t at = (vm.at >> (8 * k)) & 255u;      // 0xff: absent (KSIM_PASSED is no plugin's place)
    if (at != 255u && f == at) enter = true;
  }
  if (enter)
    select_victims<false, true, PDB, true, PreemptSpread, true, PreemptVol>(
        c, P, s, p, P.plans[st->cursor], P.uses + p.use_first, pre, node, prio, fit_index >= 0, port_mask, ds, at_ipa,
        at_pts, out, vm);
  pre.res[node] = out;
}

// VolumeBinding and VolumeZone after the removals (ksim_preempt_full, for a
// preemptor with volume groups): both verdicts depend on the node and the
// pod's groups alone, so a potential node either check fails is no candidate
// whatever its victims.  It stays a potential node (upstream counts it before
// the dry run) but leaves the candidates before k_preempt_pick scans them, so
// it does not count toward the numCandidates cut.  vb / vz: the plugin is in
// the filter list.
__global__ __launch_bounds__(256) void k_preempt_static_veto(DevCluster c, DevPods P,
                                                             const DevState* __restrict__ st, DevPreempt pre,
                                                             int32_t vb, int32_t vz) {
  const int32_t node = blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= c.n || pre.res[node].cand == 0) return;
  const ksim_pod& p = P.pods[st->cursor];
  bool bad = false;
  if (vb && p.vb_count) bad = volume_binding_fails(c, P, p.vb_first, p.vb_count, node) != 0;
  if (!bad && vz && p.vz_count) bad = !volume_groups_match(c, P, p.vz_first, p.vz_count, node);
  if (bad) pre.res[node].cand = 0;                       // the violations above bit 0 go with it
}

// The cluster-wide total of each required-affinity use over the nodes that
// carry its key (pre.afftot[i]; 0 for every other use): with the node's own
// domain sum it tells a dry run whether a matching pod exists outside the
// node's domains (upstream's len(affinityCounts) after RemovePod).
__global__ __launch_bounds__(256) void k_preempt_totals(DevCluster c, DevPods P, const DevState* __restrict__ st,
                                                        DevPreempt pre, uint32_t aff) {
  __shared__ int64_t sh[4];
  const ksim_pod& p = P.pods[st->cursor];
  const ksim_topo_use* U = P.uses + p.use_first;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int i = 0; i < KSIM_MAX_USES; i++) {
    if (!((aff >> i) & 1u)) {                          // block-uniform
      if (tid == 0) pre.afftot[i] = 0;
      continue;
    }
    const ksim_topo_use u = load_use(U, i);
    int64_t sum = 0;
    if (u.col != KSIM_COL_NONE && u.cls >= 0)
      for (int32_t n = tid; n < c.n; n += blockDim.x)
        if (c.labels[(size_t)u.col * c.n + n] != 0) sum += c.cnt[(size_t)u.cls * c.n + n];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    __syncthreads();
    if (lane == 0) sh[w] = sum;
    __syncthreads();
    if (tid == 0) pre.afftot[i] = sh[0] + sh[1] + sh[2] + sh[3];
  }
}

// TpKeyToCriticalPaths for a dry run that moves one domain: per DoNotSchedule
// spread use of the preemptor (one block each, block k = the k-th set bit of
// `hard`), over the present entries of the table load_topo_row reads,
// smin[3 i ..] = {the minimum, the value id of one arg-min, the minimum
// over the present values other than that one}; math.MaxInt32 where there is
// none.  Launched after the status pass, before k_preempt_nodes.
__global__ __launch_bounds__(256) void k_preempt_spread_mins(DevCluster c, DevPods P,
                                                             const DevState* __restrict__ st, DevScratch s,
                                                             int64_t* __restrict__ smin, uint32_t hard) {
  __shared__ int64_t sh_m[4];
  __shared__ int32_t sh_v[4];
  __shared__ int64_t s_m1;
  __shared__ int32_t s_v1;
  constexpr int64_t kNone = 2147483647;
  int i = 0;                                           // this block's use
  for (int k = blockIdx.x; i < KSIM_MAX_USES; i++)
    if (((hard >> i) & 1u) && k-- == 0) break;
  if (i >= KSIM_MAX_USES) return;
  const int32_t pi = st->cursor;
  const ksim_pod& p = P.pods[pi];
  const ksim_topo_use u = load_use(P.uses + p.use_first, i);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int32_t V = u.col != KSIM_COL_NONE ? c.col_nvals[u.col] : 0;
  const int64_t* d = ((P.plans[pi].m.ptab >> i) & 1u) ? P.ptab + u._pad : s.dom + (size_t)i * c.vmax;
  // the pair (count, value id), smallest count first, then the smallest id
  auto less = [](int64_t ma, int32_t va, int64_t mb, int32_t vb) { return ma < mb || (ma == mb && va < vb); };
  int64_t m1 = kNone, m2 = kNone;
  int32_t v1 = -1;
  for (int pass = 0; pass < 2; pass++) {               // pass 1: the same over the values other than v1
    int64_t m = kNone;
    int32_t at = INT32_MAX;
    for (int32_t v = tid; v < V; v += blockDim.x) {
      const int64_t x = d[v];
      if ((x >> kDomMarkShift) == 0 || (pass == 1 && v == v1)) continue;
      const int64_t cnt = x & kDomCountMask;
      if (less(cnt, v, m, at)) {
        m = cnt;
        at = v;
      }
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
      const int64_t mo = __shfl_xor(m, k, 64);
      const int32_t vo = __shfl_xor(at, k, 64);
      if (less(mo, vo, m, at)) {
        m = mo;
        at = vo;
      }
    }
    __syncthreads();                                    // the last pass's readers are done
    if (lane == 0) {
      sh_m[w] = m;
      sh_v[w] = at;
    }
    __syncthreads();
    if (tid == 0) {
      for (int k = 1; k < 4; k++)
        if (less(sh_m[k], sh_v[k], m, at)) {
          m = sh_m[k];
          at = sh_v[k];
        }
      s_m1 = m;
      s_v1 = at == INT32_MAX ? -1 : at;
    }
    __syncthreads();
    if (pass == 0) {
      m1 = s_m1;
      v1 = s_v1;
    } else {
      m2 = s_m1;
    }
  }
  if (tid == 0) {
    smin[3 * i] = m1;
    smin[3 * i + 1] = v1;
    smin[3 * i + 2] = m2;
  }
}

// pickOneNodeForPreemption order: a is better than b
__device__ __forceinline__ bool better(const PreemptNode& a, int32_t na, const PreemptNode& b, int32_t nb) {
  if (nb < 0) return na >= 0;
  if (na < 0) return false;
  if (a.cand != b.cand) return a.cand < b.cand;         // fewest PDB violations (both are candidates)
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
  __shared__ int32_t sh[3][kPickThreads / 64];
  __shared__ PreemptNode s_best[kPickThreads];
  __shared__ int32_t s_node[kPickThreads];
  __shared__ int32_t s_first;                            // rank of the first candidate without a PDB violation
  const int tid = threadIdx.x;
  const int32_t N = c.n, chunk = (N + kPickThreads - 1) / kPickThreads;
  const int32_t lo = min(N, tid * chunk), hi = min(N, lo + chunk);
  int32_t npot = 0, ncand = 0, nclean = 0;
  for (int32_t x = lo; x < hi; x++) {
    const int32_t cand = pre.res[x].cand;
    npot += pre.res[x].potential;
    ncand += cand & 1;
    nclean += cand == 1;                                 // a candidate without a PDB violation
  }
  if (tid == 0) s_first = -1;
  // GetOffsetAndNumCandidates over the potential nodes; dryRunPreemption keeps
  // candidates in nodeTree order until numCandidates were found and one of
  // them has no PDB violation: candidate x is cut when at least `want`
  // candidates precede it and one of those is clean.  Without PDBs every
  // candidate is clean and the rule is rank < want.  One block scan of the
  // three counts: the candidates and the clean ones before this thread's
  // chunk, and the totals.
  int32_t total_pot = 0, cexcl = 0, total_cand = 0, kexcl = 0;
  {
    const int lane = tid & 63, w = tid >> 6;
    int32_t x = npot, y = ncand, z = nclean;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int32_t a = __shfl_up(x, d, 64), b = __shfl_up(y, d, 64), e = __shfl_up(z, d, 64);
      if (lane >= d) {
        x += a;
        y += b;
        z += e;
      }
    }
    if (lane == 63) {
      sh[0][w] = x;
      sh[1][w] = y;
      sh[2][w] = z;
    }
    __syncthreads();
    for (int i = 0; i < kPickThreads / 64; i++) {
      total_pot += sh[0][i];
      total_cand += sh[1][i];
      if (i < w) {
        cexcl += sh[1][i];
        kexcl += sh[2][i];
      }
    }
    cexcl += y - ncand;
    kexcl += z - nclean;
  }
  int32_t want = total_pot * min_pct / 100;
  if (want < min_abs) want = min_abs;
  if (want > total_pot) want = total_pot;
  PreemptNode best{};
  int32_t best_node = -1, rank = cexcl, clean = kexcl;
  for (int32_t x = lo; x < hi; x++) {
    const PreemptNode& r = pre.res[x];
    if (!r.cand) continue;
    if ((rank < want || (want > 0 && clean == 0)) && better(r, x, best, best_node)) {
      best = r;
      best_node = x;
    }
    if (r.cand == 1 && clean++ == 0) s_first = rank;    // one thread holds the first clean candidate
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
    // kept: the first `want` candidates, or up to the first clean one when that comes later
    // (all of them when none is clean)
    const int32_t upto = s_first < 0 ? total_cand : s_first + 1;
    int32_t kept = want > upto ? want : upto;
    if (kept > total_cand) kept = total_cand;
    pre.pick[0] = s_node[0];
    pre.pick[1] = s_node[0] >= 0 ? s_best[0].nv : 0;
    pre.pick[2] = total_pot;
    pre.pick[3] = want > 0 ? kept : 0;
    pre.pick[4] = s_node[0] >= 0 ? s_best[0].nviol() : 0;
  }
}

void launch_preempt(const LaunchArgs& a, const DevPreempt& pre, int32_t fit_index, int32_t prio,
                    hipStream_t stream, bool filter, int32_t port_index, uint32_t port_mask, int32_t ipa_index,
                    uint32_t aff, uint32_t anti, uint32_t exist, int32_t pts_index, uint32_t hard, int64_t* smin) {
  const int blocks = (a.c.n + 255) / 256;
  if (filter) launch_filter_only(a, stream);             // the filter statuses of every node
  if (port_index < 0) port_mask = 0;                     // no NodePorts in the profile: port uses are ignored
  if (ipa_index < 0) aff = anti = exist = 0;             // nor the InterPodAffinity uses without that filter
  if (pts_index < 0) hard = 0;                           // nor the DoNotSchedule spread uses without PodTopologySpread
  const PreemptDom dm{aff, anti, exist, ipa_index};
  const bool dom = (aff | anti | exist) != 0, pdb = pre.poff != nullptr;
  if (aff) k_preempt_totals<<<1, 256, 0, stream>>>(a.c, a.P, a.st, pre, aff);
  if (hard) {                                            // the spread form
    PreemptSpread ds{};
    static_cast<PreemptDom&>(ds) = dm;
    ds.hard = hard;
    ds.pts_index = pts_index;
    ds.smin = smin;
    k_preempt_spread_mins<<<__builtin_popcount(hard), 256, 0, stream>>>(a.c, a.P, a.st, a.s, smin, hard);
    auto nodes = pdb ? k_preempt_nodes<true, true, true> : k_preempt_nodes<true, false, true>;
    nodes<<<blocks, 256, 0, stream>>>(a.c, a.P, a.st, a.s, pre, fit_index, prio, port_index, port_mask, ds);
  } else {
    auto nodes = dom ? (pdb ? k_preempt_nodes<true, true> : k_preempt_nodes<true, false>)
                     : (pdb ? k_preempt_nodes<false, true> : k_preempt_nodes<false, false>);
    nodes<<<blocks, 256, 0, stream>>>(a.c, a.P, a.st, a.s, pre, fit_index, prio, port_index, port_mask, dm);
  }
  k_preempt_pick<<<1, kPickThreads, 0, stream>>>(a.c, pre, a.prof.preempt_min_pct, a.prof.preempt_min_abs);
}

void launch_preempt_volumes(const LaunchArgs& a, const DevPreempt& pre, int32_t fit_index, int32_t prio,
                            hipStream_t stream, int32_t port_index, uint32_t port_mask, const PreemptVol& vm) {
  const int blocks = (a.c.n + 255) / 256;
  if (port_index < 0) port_mask = 0;                     // no NodePorts in the profile: port uses are ignored
  auto nodes = pre.poff != nullptr ? k_preempt_nodes_vol<true> : k_preempt_nodes_vol<false>;
  nodes<<<blocks, 256, 0, stream>>>(a.c, a.P, a.st, a.s, pre, fit_index, prio, port_index, port_mask, vm);
  k_preempt_pick<<<1, kPickThreads, 0, stream>>>(a.c, pre, a.prof.preempt_min_pct, a.prof.preempt_min_abs);
}

void launch_preempt_full(const LaunchArgs& a, const DevPreempt& pre, int32_t fit_index, int32_t prio,
                         hipStream_t stream, int32_t port_index, uint32_t port_mask, int32_t ipa_index, uint32_t aff,
                         uint32_t anti, uint32_t exist, int32_t pts_index, uint32_t hard, int64_t* smin,
                         const PreemptVol& vm, bool vb, bool vz) {
  const int blocks = (a.c.n + 255) / 256;
  if (port_index < 0) port_mask = 0;                     // as launch_preempt: a use whose filter the profile lacks
  if (ipa_index < 0) aff = anti = exist = 0;             // is in none of the masks
  if (pts_index < 0) hard = 0;
  PreemptSpread ds{};
  ds.aff = aff;
  ds.anti = anti;
  ds.exist = exist;
  ds.ipa_index = ipa_index;
  ds.hard = hard;
  ds.pts_index = pts_index;
  ds.smin = smin;
  if (aff) k_preempt_totals<<<1, 256, 0, stream>>>(a.c, a.P, a.st, pre, aff);
  if (hard) k_preempt_spread_mins<<<__builtin_popcount(hard), 256, 0, stream>>>(a.c, a.P, a.st, a.s, smin, hard);
  auto nodes = pre.poff != nullptr ? k_preempt_nodes_full<true> : k_preempt_nodes_full<false>;
  nodes<<<blocks, 256, 0, stream>>>(a.c, a.P, a.st, a.s, pre, fit_index, prio, port_index, port_mask, ds, vm);
  if (vb || vz) k_preempt_static_veto<<<blocks, 256, 0, stream>>>(a.c, a.P, a.st, pre, vb, vz);
  k_preempt_pick<<<1, kPickThreads, 0, stream>>>(a.c, pre, a.prof.preempt_min_pct, a.prof.preempt_min_abs);
}

void launch_preempt_veto(const LaunchArgs& a, const DevPreempt& pre, hipStream_t stream, bool vb, bool vz) {
  const int blocks = (a.c.n + 255) / 256;
  k_preempt_static_veto<<<blocks, 256, 0, stream>>>(a.c, a.P, a.st, pre, vb, vz);
  k_preempt_pick<<<1, kPickThreads, 0, stream>>>(a.c, pre, a.prof.preempt_min_pct, a.prof.preempt_min_abs);
}

}  // namespace ksim
