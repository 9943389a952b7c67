// ksim_preempt.hip — PostFilter: DefaultPreemption's dry run on the device
// (upstream preemption.go / default_preemption.go, v1.26).
//
// After an unschedulable cycle, every node where preemption might help (its
// first failing filter returned plain Unschedulable and the dry run re-runs it)
// runs SelectVictimsOnNode on its own thread: remove every bound pod of lower
// priority, check the pod fits, then reprieve the removed pods most important
// first (priority desc, start time asc), keeping each one the pod still fits
// beside.  The bound pods are held per node in importance order (CSR), so the
// lower-priority pods are a suffix of the node's range.  With
// PodDisruptionBudgets on the table (ksim_set_bound_pod_pdbs) the thread first
// splits that suffix as filterPodsWithPDBViolation does and reprieves the
// violating rows first (PDB, a template parameter of its own).
//
// The thread's trial state is made of sides.  Each owns its registers and has
// init (its start on the node), move (one row in or out), move_group (the
// node's nominated group in) and fails (the filters it re-runs):
//   RequestSide  the node's requests; NodeResourcesFit
//   PortSide     the node's count of each port class of the preemptor's, from the
//                rows' class contributions (ksim_set_bound_pod_adds); NodePorts
//   RowSide      the node's TopoRow, moved by the same contributions; NodePorts,
//                InterPodAffinity and, with SPREAD, PodTopologySpread against the
//                minimum over the other present domains (k_preempt_spread_mins)
//   VolSide      the node's attached volumes per family, moved by the rows'
//                holdings (ksim_set_bound_pod_volumes); the node volume limit
//                plugins.  A shared volume's holder count lives in the side
//                beside it: PortSide's held[] or the TopoRow's own entry.
// A form lists the sides one kind of preemptor needs and says which first
// failing filters make a potential node.  Each has kernels and a kernel
// argument of its own, so a preemptor without a kind of use runs the code and
// keeps the registers of the form without it:
//   FreeForm     request                  no filter-read uses
//   PortsForm    request, ports           host ports (in FreeForm's kernels, behind one uniform branch)
//   DomForm      request, row             required pod (anti-)affinity
//   SpreadForm   request, row + SPREAD    DoNotSchedule spread (ksim_preempt_spread)
//   VolumeForm   request, ports, volume   counted volumes (ksim_preempt_volumes)
//   FullForm     request, row + SPREAD, volume   volumes beside affinity or spread (ksim_preempt_full)
// For a preemptor with volume groups k_preempt_static_veto then takes the nodes
// VolumeBinding or VolumeZone fails out of the candidates.  One block keeps
// candidates in nodeTree order (upstream scans from a random offset; offset 0
// here) until numCandidates were found and one of them has no PDB violation,
// and picks one by pickOneNodeForPreemption's criteria.
//
// The batched dry run (ksim_preempt_many) answers many preemptors against one
// snapshot: k_preempt_many_nodes runs the forms without a row side on a grid of
// (node block, preemptor), each preemptor on result and flag slabs of its own
// (two preemptors of different priority clear and mark different rows of one
// node), with the filter status computed in the kernel instead of a filter
// pass of its own; k_preempt_pick runs one block per preemptor, and
// k_preempt_many_victims compacts each nominated node's victims on the device.
// select_victims is the same code for both: a trial reads its pod, priority
// and slabs through its PreemptCommon, the handle's own in k_preempt_nodes and
// the row's view in k_preempt_many_nodes.  ksim_preempt_many_dom also batches
// the preemptors with a row side: each gets a PreFilter state of its own for
// the call (k_preempt_many_dom: its domain tables, affinity totals and
// topology flags; k_preempt_many_mins: its critical-path minima), and
// k_preempt_many_dom_nodes runs SpreadForm or FullForm through a row's view
// that also swaps those in.
//
// ksim_preempt_commit makes a dry run's evictions real on the device: the
// k_commit_* kernels below ("committed preemption").
#include "ksim_device.h"
#include "ksim_internal.h"
#include "ksim_wave.h"

#include <type_traits>

namespace ksim {

// The arguments every form's node kernel takes.  fit_index / port_index:
// NodeResourcesFit's and NodePorts' places in the filter list (-1: absent);
// port_mask: the preemptor's NodePorts uses (bit i = use i).
struct PreemptCommon {
  DevCluster c;
  DevPods P;
  const DevState* st;
  DevScratch s;
  DevPreempt pre;
  int32_t fit_index, prio, port_index;
  uint32_t port_mask;
};
// The preemptor's filter-read uses in the domain form (kernel argument, bit i =
// use i): its InterPodAffinity uses by role, and that filter's place in the
// profile.
struct PreemptDom {
  uint32_t aff, anti, exist;
  int32_t ipa_index;
};
// The spread form's argument: the preemptor's DoNotSchedule spread uses,
// PodTopologySpread's place, and per use {the minimum over the present
// domains, the value id of one arg-min, the minimum over the others}
// (k_preempt_spread_mins; [KSIM_MAX_USES][3]).
struct PreemptSpread : PreemptDom {
  uint32_t hard;
  int32_t pts_index;
  int64_t* smin;
};
// The full form's: hard may be empty (volumes beside affinity alone); then no
// use is a spread use and PodTopologySpread's place is not read.
struct PreemptFull {
  PreemptSpread ds;
  PreemptVol vm;
};

// One node's dry run: what the sides read beside their own state.  g: the
// node's nominated group (-1: none); [j0, b): the rows of lower priority than
// the preemptor's.
struct Trial {
  const PreemptCommon& a;
  const ksim_pod& p;
  const PodPlan& plan;
  const ksim_topo_use* U;
  int32_t node, g, j0, b;
};

// The first failing filter is NodeResourcesFit or, for a preemptor with port
// uses, NodePorts: a potential node in every form.
__device__ __forceinline__ bool failed_fit_or_ports(uint32_t f, const PreemptCommon& a) {
  return (a.fit_index >= 0 && f == (uint32_t)a.fit_index) || (a.port_mask && f == (uint32_t)a.port_index);
}

// NodeInfo.AddPod / RemovePod (and PreFilterExtensions' of the same names) on
// per-use counts: sign x count of every add of [e0, e1) whose class one of the
// preemptor's uses reads.  cls[i]: that class, kNoPortClass for a use no add
// moves (no add carries it), block-uniform.
constexpr int32_t kNoPortClass = -2;
template <class T>
__device__ __forceinline__ void count_add(T (&n)[KSIM_MAX_USES], const int32_t (&cls)[KSIM_MAX_USES],
                                          const ksim_class_add* __restrict__ adds, int32_t e0, int32_t e1, int sign) {
  for (int32_t e = e0; e < e1; e++) {
    const ksim_class_add x = adds[e];
#pragma unroll
    for (int i = 0; i < KSIM_MAX_USES; i++)
      if (cls[i] == x.cls) n[i] += (T)sign * x.count;
  }
}

// ---- the request side ----------------------------------------------------------
__device__ __forceinline__ void row_add_req(NodeRow& r, const int64_t* q, int sign, int n_scalar) {
  r.req_cpu += sign * q[0];
  r.req_mem += sign * q[1];
  r.req_eph += sign * q[2];
#pragma unroll
  for (int k = 0; k < KSIM_MAX_SCALAR; k++)
    if (k < n_scalar) r.req_sc[k] += sign * q[3 + k];
  r.num_pods += sign;
}
struct RequestSide {
  NodeRow r;
  __device__ __forceinline__ void init(const Trial& x) { r = load_row(x.a.c, x.node); }
  __device__ __forceinline__ void move(const Trial& x, int32_t j, int sign) {
    row_add_req(r, x.a.pre.req + (size_t)j * KSIM_PREEMPT_REQ, sign, x.a.c.n_scalar);
  }
  __device__ __forceinline__ void move_group(const Trial& x) {   // the nominated pods stay (pass 1)
    const int64_t* q = x.a.pre.nreq + (size_t)x.g * (KSIM_PREEMPT_REQ + 1);
    row_add_req(r, q, 1, x.a.c.n_scalar);
    r.num_pods += (int32_t)q[KSIM_PREEMPT_REQ] - 1;
  }
  // alone: the form re-runs no other filter; one that does re-runs NodeResourcesFit only when the profile has it
  __device__ __forceinline__ bool fails(const Trial& x, bool alone = false) const {
    return (alone || x.a.fit_index >= 0) && fits_request(r, x.p, x.a.c.n_scalar, x.a.c.fit_ignore) != 0;
  }
};

// ---- the ports side ------------------------------------------------------------
// held[i] = pods on the node of port use i's class (0 for every other use; the
// volume side keeps a shared volume's holders in the entry of its use).
struct PortSide {
  int32_t cls[KSIM_MAX_USES];
  int32_t held[KSIM_MAX_USES];
  __device__ __forceinline__ void init(const Trial& x) {
#pragma unroll
    for (int i = 0; i < KSIM_MAX_USES; i++) {
      cls[i] = kNoPortClass;
      held[i] = 0;
      if ((x.a.port_mask >> i) & 1u) {
        cls[i] = load_use(x.U, i).cls;
        held[i] = (int32_t)class_count(x.a.c, cls[i], x.node);
      }
    }
  }
  __device__ __forceinline__ void move(const Trial& x, int32_t j, int sign) {
    count_add(held, cls, x.a.pre.adds, x.a.pre.aoff[j], x.a.pre.aoff[j + 1], sign);
  }
  __device__ __forceinline__ void move_group(const Trial& x) {
    count_add(held, cls, x.a.pre.gadds, x.a.pre.goff[x.g], x.a.pre.goff[x.g + 1], 1);
  }
  // nodeports Filter.  among: the port uses, for a form whose volume side keeps
  // its holders here (a held volume class is no conflict)
  __device__ __forceinline__ bool fails(uint32_t among = ~0u) const {
    bool hit = false;
#pragma unroll
    for (int i = 0; i < KSIM_MAX_USES; i++)
      if (((among >> i) & 1u) && held[i] > 0) hit = true;
    return hit;
  }
};

// ---- the row side --------------------------------------------------------------
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
// The node's TopoRow under the roles the dry run's filters read (mm): ports,
// affinity and spread counts move by the class adds.  A use whose key the node
// lacks (t.v[i] == 0) moves too, but no Filter reads its count.  SPREAD:
// PodTopologySpread is re-run as well.  In node n's dry run only n's pods move,
// so per constraint only the count of n's own domain moves and the critical
// path is min(own count, others_i): the minimum over the other present domains
// (dm.smin: the second minimum when n's value is the arg-min), fixed for the
// dry run and folded into thr[i].  A DoNotSchedule use's entry carries the
// presence marks above its count (kDomMarkShift); the count never goes below
// zero, so adding to the whole entry leaves them alone.  A pod of n moves
// constraint i only when n is eligible for it (every hard constraint's key on
// n, and n passes i's node inclusion policies, as k_topo_prefilter counted;
// cls[i] is kNoPortClass elsewhere: updateWithPod) and elsewhere the verdict is
// the status pass's.
template <bool SPREAD>
struct RowSide {
  using Args = std::conditional_t<SPREAD, PreemptSpread, PreemptDom>;
  TopoRow t;
  int32_t cls[KSIM_MAX_USES];
  UseMasks mm;
  bool outside;
  uint32_t elig, over;                                  // SPREAD: the hard uses this node's pods move; spread_filter
  int64_t thr[KSIM_MAX_USES];                           // SPREAD: per hard use, the count the row may reach

  // A node that failed InterPodAffinity or PodTopologySpread is a potential
  // node only for an anti-affinity / the skew reason (resolvable, below).
  static __device__ __forceinline__ bool potential(uint32_t f, const PreemptCommon& a, const Args& dm, bool& at_ipa,
                                                   bool& at_pts) {
    at_ipa = (dm.aff | dm.anti | dm.exist) != 0 && f == (uint32_t)dm.ipa_index;
    if constexpr (SPREAD) at_pts = dm.hard != 0 && f == (uint32_t)dm.pts_index;
    return failed_fit_or_ports(f, a) || at_ipa || at_pts;
  }
  __device__ __forceinline__ void init(const Trial& x, const Args& dm) {
    mm = UseMasks{};
    mm.port = x.a.port_mask;
    mm.aff = dm.aff;
    mm.anti = dm.anti;
    mm.exist = dm.exist;
    outside = false;
    elig = over = 0;
    const uint32_t read = x.a.port_mask | dm.aff | dm.anti | dm.exist;
    load_topo_row(x.a.c, x.U, x.p.use_count, x.plan.m, x.a.s, x.a.P.ptab, x.node, t);
    if constexpr (SPREAD) {                             // updateWithPod's node tests, once per node
      bool all_hard = true;                             // nodeLabelsMatchSpreadConstraints
#pragma unroll
      for (int i = 0; i < KSIM_MAX_USES; i++)
        if (((dm.hard >> i) & 1u) && t.v[i] == 0) all_hard = false;
      if (all_hard) {                                   // matchNodeInclusionPolicies, as k_topo_prefilter
        const UseMasks& m = x.plan.m;
        const bool aff_ok = (m.honor_aff & dm.hard) ? required_node_affinity_match(x.a.c, x.a.P, x.p, x.node) : true;
        const bool taint_ok = (m.honor_taints & dm.hard) ? !node_has_untolerated_taint(x.a.c, x.p, x.node) : true;
        elig = dm.hard & ~(aff_ok ? 0u : m.honor_aff) & ~(taint_ok ? 0u : m.honor_taints);
      }
    }
#pragma unroll
    for (int i = 0; i < KSIM_MAX_USES; i++) {
      cls[i] = kNoPortClass;
      if ((read >> i) & 1u) cls[i] = load_use(x.U, i).cls;
      if (((dm.aff >> i) & 1u) && t.v[i] != 0 && x.a.pre.afftot[i] - t.x[i] > 0) outside = true;
      if constexpr (SPREAD) {
        thr[i] = 0;
        if ((dm.hard >> i) & 1u) {
          const int64_t* mn = dm.smin + 3 * i;          // {min1, the arg-min's value id, min2}
          const ksim_topo_use u = load_use(x.U, i);
          const bool mine = (elig >> i) & 1u;
          // others_i(n): the second minimum when n's own domain is the arg-min
          const int64_t oth = mine && (int64_t)t.v[i] == mn[1] ? mn[2] : mn[0];
          const int64_t lim = (int64_t)((x.plan.m.self_match >> i) & 1u) - (int64_t)u.arg;
          thr[i] = oth - lim;
          if (mine && lim > 0) over |= 1u << i;
          if (mine) cls[i] = u.cls;
        }
      }
    }
  }
  __device__ __forceinline__ void move(const Trial& x, int32_t j, int sign) {
    count_add(t.x, cls, x.a.pre.adds, x.a.pre.aoff[j], x.a.pre.aoff[j + 1], sign);
  }
  __device__ __forceinline__ void move_group(const Trial& x, const Args&) {
    count_add(t.x, cls, x.a.pre.gadds, x.a.pre.goff[x.g], x.a.pre.goff[x.g + 1], 1);
  }
  // The status pass's detail, re-derived from the row (with the nominated group
  // on it: pass 1): false for UnschedulableAndUnresolvable, no potential node.
  __device__ __forceinline__ bool resolvable(const Trial& x, const Args& dm, bool at_ipa, bool at_pts) const {
    if constexpr (SPREAD) {
      if (at_pts && spread_filter(dm.hard, over, thr, t) == KSIM_PTS_MISSING_LABEL) return false;
    }
    if (at_ipa) {
      const uint32_t why = ipa_filter(mm, x.p, affinity_flags(dm.aff, outside, t), t);
      if (why != KSIM_IPA_ANTI_AFFINITY && why != KSIM_IPA_EXISTING_ANTI) return false;
    }
    return true;
  }
  __device__ __forceinline__ bool fails(const Trial& x, const Args& dm) const {
    if constexpr (SPREAD) {
      if (spread_fails(dm.hard, over, thr, t)) return true;
    }
    return node_port_conflict(mm, t) || ipa_filter(mm, x.p, affinity_flags(dm.aff, outside, t), t) != 0;
  }
};

// ---- the volume side -----------------------------------------------------------
// Pods of the node's suffix [j0, b) that are out of the trial state (bit 0 of
// their flag; row `skip` apart) and hold volume class `cls`: a direct count,
// quadratic in the node's victims like the PDB split's.
__device__ __forceinline__ int32_t vol_out_holders(const Trial& x, const PreemptVol& vm, int32_t skip, int32_t cls) {
  int32_t n = 0;
  for (int32_t k = x.j0; k < x.b; k++) {
    if (k == skip || !(x.a.pre.vflag[k] & 1)) continue;
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
// The node's attached volumes per family of the preemptor's (att, c.vol_attached
// moved with every pod taken out or put back) and their limits, the family of
// each volume use (ufam, four bits each) and per family the preemptor's
// classless volumes (own).  A shared volume the preemptor mounts is a count
// class; the node's holders of it are hv.held[i] under hv.cls[i], both in the
// side the form keeps beside this one and hands in (Holders; the ids are
// disjoint from the port and selector classes, and no add names one; a
// classless volume use keeps kNoPortClass).  Everything is indexed by unrolled
// constants only, so it stays in registers.
template <class H>
struct Holders {
  int32_t (&cls)[KSIM_MAX_USES];
  H (&held)[KSIM_MAX_USES];
};
struct VolSide {
  int64_t att[KSIM_MAX_VOL_FAMILIES];
  int32_t lim[KSIM_MAX_VOL_FAMILIES];
  uint64_t ufam;
  int64_t own[KSIM_MAX_VOL_FAMILIES];

  // the first failing filter is one of the four limit plugins (at: their places; they return plain Unschedulable)
  static __device__ __forceinline__ bool potential(uint32_t f, const PreemptVol& vm) {
    bool hit = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t at = (vm.at >> (8 * k)) & 255u;      // 0xff: absent (KSIM_PASSED is no plugin's place)
      if (at != 255u && f == at) hit = true;
    }
    return hit;
  }
  template <class H>
  __device__ __forceinline__ void init(const Trial& x, const PreemptVol& vm, const Holders<H>& hv) {
    ufam = 0;
#pragma unroll
    for (int k = 0; k < KSIM_MAX_VOL_FAMILIES; k++) {
      own[k] = 0;
      att[k] = 0;
      lim[k] = 2147483647;
      if ((vm.fams >> k) & 1u) {
        att[k] = x.a.c.vol_attached[(size_t)k * x.a.c.n + x.node];
        lim[k] = x.a.c.vol_limit[(size_t)k * x.a.c.n + x.node];
      }
    }
#pragma unroll
    for (int i = 0; i < KSIM_MAX_USES; i++) {
      if (!((vm.uses >> i) & 1u)) continue;
      const ksim_topo_use u = load_use(x.U, i);          // the device copy: family in _pad
      ufam |= (uint64_t)(u._pad & 15) << (4 * i);
      if (u.cls >= 0) {
        hv.cls[i] = u.cls;
        hv.held[i] = (H)class_count(x.a.c, u.cls, x.node);    // (a TopoRow's entry of a volume use holds just that)
      } else {
#pragma unroll
        for (int k = 0; k < KSIM_MAX_VOL_FAMILIES; k++)
          if (k == u._pad) own[k] += u.arg;
      }
    }
  }
  // NodeInfo.AddPod / RemovePod on the node's attached volumes (volume_bind's
  // rule on the thread's copy): the holdings [e0, e1) of one pod.  A classless
  // holding moves its family's count by arg.  A class holding moves it by one
  // when no other pod on the node holds the volume: for a class of the
  // preemptor's that is hv.held[i] (moved here too), for any other class
  // others(cls, e) counts the other holders.  Families the preemptor has no use
  // of are not read.
  template <class H, typename OTHERS>
  __device__ __forceinline__ void add(const PreemptVol& vm, const Holders<H>& hv, const VolHold* __restrict__ ents,
                                      int32_t e0, int32_t e1, int sign, OTHERS others) {
    for (int32_t e = e0; e < e1; e++) {
      const VolHold x = ents[e];
      if (!((vm.fams >> x.fam) & 1u)) continue;
      int64_t d = (int64_t)sign * x.arg;
      if (x.cls >= 0) {
        bool mine = false;
        int32_t rest = 0;                                  // the volume's other holders on the node
#pragma unroll
        for (int i = 0; i < KSIM_MAX_USES; i++)
          if (((vm.uses >> i) & 1u) && hv.cls[i] == x.cls) {
            mine = true;
            rest = (int32_t)(sign < 0 ? hv.held[i] - 1 : hv.held[i]);
            hv.held[i] += sign;
          }
        if (!mine) rest = others(x.cls, e);
        d = rest == 0 ? sign : 0;
      }
#pragma unroll
      for (int k = 0; k < KSIM_MAX_VOL_FAMILIES; k++)
        if (k == x.fam) att[k] += d;
    }
  }
  // Row j's holdings.  The holders of a class the preemptor does not use, row j
  // apart: the device's count (every bound holder of the node, whatever its
  // priority, row j among them) and the nominated group's, less the rows that
  // are out.
  template <class H>
  __device__ __forceinline__ void move(const Trial& x, const PreemptVol& vm, const Holders<H>& hv, int32_t j, int sign) {
    add(vm, hv, vm.vols, vm.voff[j], vm.voff[j + 1], sign, [&](int32_t cl, int32_t) {
      const int32_t grp = x.g >= 0 ? vol_class_entries(vm.gvols, vm.gvoff[x.g], vm.gvoff[x.g + 1], cl) : 0;
      return (int32_t)class_count(x.a.c, cl, x.node) - 1 + grp - vol_out_holders(x, vm, j, cl);
    });
  }
  // The group's volumes, each pod after the ones before it
  template <class H>
  __device__ __forceinline__ void move_group(const Trial& x, const PreemptVol& vm, const Holders<H>& hv) {
    const int32_t g0 = vm.gvoff[x.g];
    add(vm, hv, vm.gvols, g0, vm.gvoff[x.g + 1], 1, [&](int32_t cl, int32_t e) {
      return class_count(x.a.c, cl, x.node) + vol_class_entries(vm.gvols, g0, e, cl);
    });
  }
  // nodevolumelimits Filter on the moved counts (volume_limit_fails' rule, 64-bit
  // sums): per family of the preemptor's, new = its classless volumes (own[f])
  // plus its class volumes no pod left on the node holds.
  template <class H>
  __device__ __forceinline__ bool fails(const PreemptVol& vm, const Holders<H>& hv) const {
    bool bad = false;
#pragma unroll
    for (int k = 0; k < KSIM_MAX_VOL_FAMILIES; k++) {
      if (!((vm.fams >> k) & 1u)) continue;
      int64_t add = own[k];
#pragma unroll
      for (int i = 0; i < KSIM_MAX_USES; i++)
        if (((vm.uses >> i) & 1u) && hv.cls[i] >= 0 && (int)((ufam >> (4 * i)) & 15u) == k) add += hv.held[i] == 0;
      const bool csi = (vm.csi >> k) & 1u;
      if (lim[k] != 2147483647 && att[k] + add > (int64_t)lim[k] && (!csi || add > 0)) bad = true;
    }
    return bad;
  }
};

// ---- the forms -----------------------------------------------------------------
// Args: the form's kernel argument.  potential(): the node's first failing
// filter is one the form re-runs (at_ipa / at_pts: InterPodAffinity's /
// PodTopologySpread's, whose detail resolvable() then asks for).  init(): side
// by side, its start and then the node's nominated group (the nominated pods
// stay: pass 1).  fails(): false = the pod passes; a form that re-runs another
// filter re-runs NodeResourcesFit only when the profile has it.  kOut:
// bit 0 of a row's flag says "out of the trial state" during the trials too
// (the volume side reads it).
template <class SIDE, class... A>
__device__ __forceinline__ void start(SIDE& side, const Trial& x, const A&... a) {
  side.init(x, a...);
  if (x.g >= 0) side.move_group(x, a...);
}
struct FormBase {
  static constexpr uint8_t kOut = 0;
  RequestSide req;
  template <class A>
  __device__ __forceinline__ bool resolvable(const Trial&, const A&, bool, bool) const {
    return true;
  }
};
struct FreeForm : FormBase {
  using Args = PreemptDom;                               // not read
  static __device__ __forceinline__ bool potential(uint32_t f, const PreemptCommon& a, const Args&, bool&, bool&) {
    return failed_fit_or_ports(f, a);
  }
  __device__ __forceinline__ void init(const Trial& x, const Args&) { start(req, x); }
  __device__ __forceinline__ void move_row(const Trial& x, const Args&, int32_t j, int sign) { req.move(x, j, sign); }
  __device__ __forceinline__ bool fails(const Trial& x, const Args&) { return req.fails(x, true); }
};
struct PortsForm : FormBase {                            // (FreeForm's kernels and potential nodes)
  using Args = FreeForm::Args;
  PortSide ports;
  __device__ __forceinline__ void init(const Trial& x, const Args&) {
    start(req, x);
    start(ports, x);
  }
  __device__ __forceinline__ void move_row(const Trial& x, const Args&, int32_t j, int sign) {
    req.move(x, j, sign);
    ports.move(x, j, sign);
  }
  __device__ __forceinline__ bool fails(const Trial& x, const Args&) {
    return req.fails(x) || ports.fails();
  }
};
template <bool SPREAD>
struct RowForm : FormBase {
  using Args = typename RowSide<SPREAD>::Args;
  RowSide<SPREAD> row;
  static constexpr auto potential = &RowSide<SPREAD>::potential;
  __device__ __forceinline__ void init(const Trial& x, const Args& dm) {
    start(req, x);
    start(row, x, dm);
  }
  __device__ __forceinline__ bool resolvable(const Trial& x, const Args& dm, bool at_ipa, bool at_pts) const {
    return row.resolvable(x, dm, at_ipa, at_pts);
  }
  __device__ __forceinline__ void move_row(const Trial& x, const Args&, int32_t j, int sign) {
    req.move(x, j, sign);
    row.move(x, j, sign);
  }
  __device__ __forceinline__ bool fails(const Trial& x, const Args& dm) {
    return req.fails(x) || row.fails(x, dm);
  }
};
using DomForm = RowForm<false>;
using SpreadForm = RowForm<true>;
// The ports side moves only for a preemptor with port uses (port_mask,
// block-uniform); its held[] keeps the shared volumes' holders either way.
struct VolumeForm : FormBase {
  using Args = PreemptVol;
  static constexpr uint8_t kOut = 1;
  PortSide ports;
  VolSide vol;
  __device__ __forceinline__ Holders<int32_t> hv() { return {ports.cls, ports.held}; }
  static __device__ __forceinline__ bool potential(uint32_t f, const PreemptCommon& a, const Args& vm, bool&, bool&) {
    return failed_fit_or_ports(f, a) || VolSide::potential(f, vm);
  }
  __device__ __forceinline__ void init(const Trial& x, const Args& vm) {
    start(req, x);
    ports.init(x);
    vol.init(x, vm, hv());
    if (x.g >= 0 && x.a.port_mask) ports.move_group(x);
    if (x.g >= 0) vol.move_group(x, vm, hv());
  }
  __device__ __forceinline__ void move_row(const Trial& x, const Args& vm, int32_t j, int sign) {
    req.move(x, j, sign);
    if (x.a.port_mask) ports.move(x, j, sign);
    vol.move(x, vm, hv(), j, sign);
  }
  __device__ __forceinline__ bool fails(const Trial& x, const Args& vm) {
    return req.fails(x) || ports.fails(x.a.port_mask) || vol.fails(vm, hv());
  }
};
// One TopoRow, moved by the rows' class adds, and the volume side, moved by
// their holdings; a shared volume's holder count is the row's own entry of the
// volume use (load_topo_row put the node's class count there, and no add names
// a volume class, so only the volume side moves it).
struct FullForm : FormBase {
  using Args = PreemptFull;
  static constexpr uint8_t kOut = 1;
  RowSide<true> row;
  VolSide vol;
  __device__ __forceinline__ Holders<int64_t> hv() { return {row.cls, row.t.x}; }
  static __device__ __forceinline__ bool potential(uint32_t f, const PreemptCommon& a, const Args& fa, bool& at_ipa,
                                                   bool& at_pts) {
    const bool at_row = RowSide<true>::potential(f, a, fa.ds, at_ipa, at_pts);
    return at_row || VolSide::potential(f, fa.vm);
  }
  __device__ __forceinline__ void init(const Trial& x, const Args& fa) {
    start(req, x);
    start(row, x, fa.ds);
    start(vol, x, fa.vm, hv());
  }
  __device__ __forceinline__ bool resolvable(const Trial& x, const Args& fa, bool at_ipa, bool at_pts) const {
    return row.resolvable(x, fa.ds, at_ipa, at_pts);
  }
  __device__ __forceinline__ void move_row(const Trial& x, const Args& fa, int32_t j, int sign) {
    req.move(x, j, sign);
    row.move(x, j, sign);
    vol.move(x, fa.vm, hv(), j, sign);
  }
  __device__ __forceinline__ bool fails(const Trial& x, const Args& fa) {
    return req.fails(x) || row.fails(x, fa.ds) || vol.fails(fa.vm, hv());
  }
};

// SelectVictimsOnNode of one potential node, in the form's trial state.
// PDB: the table carries budgets (pre.poff / pids / pallowed).
// filterPodsWithPDBViolation walks the suffix most important first with a
// fresh copy of every budget and decrements each budget a pod matches; the pod
// violates when one of them went below zero, i.e. when the rows of [j0, j]
// that carry the budget outnumber its disruptionsAllowed.  That count is taken
// directly (quadratic in the node's victims, no per-thread array, no cap on
// the number of budgets).  The violating rows are reprieved first, then the
// others, so the victims list need not be sorted by priority: `high` is the
// first victim appended, `early` follows the true maximum priority.
// Bit 0 of a row's flag: "victim" at the end and, in a form with kOut, "out of
// the trial state" from the row's removal on (the PDB split keeps it, a reprieve clears it).
template <class FORM, bool PDB>
__device__ __forceinline__ void select_victims(Trial& x, const typename FORM::Args& fa, bool at_ipa, bool at_pts,
                                               PreemptNode& out) {
  const DevPreempt& pre = x.a.pre;
  const int32_t a = pre.off[x.node], b = pre.off[x.node + 1];
  int32_t j0 = a;
  while (j0 < b && pre.prio[j0] >= x.a.prio) j0++;     // lower priorities: the suffix [j0, b)
  for (int32_t j = a; j < j0; j++) pre.vflag[j] = 0;   // no stale flags from an earlier preemptor
  x.j0 = j0, x.b = b, x.g = pre.nslot ? pre.nslot[x.node] : -1;
  FORM t;
  t.init(x, fa);
  if (!t.resolvable(x, fa, at_ipa, at_pts)) return;     // the status pass's detail: UnschedulableAndUnresolvable
  out.potential = 1;
  if (FORM::kOut)
    for (int32_t j = j0; j < b; j++) pre.vflag[j] = 0;   // nobody is out yet
  for (int32_t j = j0; j < b; j++) {
    t.move_row(x, fa, j, -1);
    if (FORM::kOut) pre.vflag[j] = FORM::kOut;
  }
  if (!t.fails(x, fa)) {
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
        pre.vflag[j] = (viol ? kPreemptViolating : 0) | FORM::kOut;
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
        t.move_row(x, fa, j, 1);
        const bool victim = t.fails(x, fa);
        pre.vflag[j] = (uint8_t)victim | mark;
        if (victim) {
          t.move_row(x, fa, j, -1);
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
// highest-priority victims}; vflag marks the victims (bit 0) and, with PDB,
// the violating rows (bit 1), in CSR order.  One instantiation per form and
// PDB, each a code object of its own; FreeForm's also runs PortsForm, behind
// one branch on the kernel argument port_mask.
template <class FORM, bool PDB>
__global__ __launch_bounds__(256) void k_preempt_nodes(PreemptCommon a, typename FORM::Args fa) {
  const int32_t node = blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= a.c.n) return;
  PreemptNode out{};
  const uint32_t f = a.s.fail[node];
  const ksim_pod& p = a.P.pods[a.st->cursor];
  Trial x{a, p, a.P.plans[a.st->cursor], a.P.uses + p.use_first, node, -1, 0, 0};
  bool at_ipa = false, at_pts = false;
  if (FORM::potential(f, a, fa, at_ipa, at_pts)) {
    if constexpr (std::is_same_v<FORM, FreeForm>) {
      if (a.port_mask)                                   // kernel argument: one uniform branch
        select_victims<PortsForm, PDB>(x, fa, at_ipa, at_pts, out);
      else
        select_victims<FreeForm, PDB>(x, fa, at_ipa, at_pts, out);
    } else {
      select_victims<FORM, PDB>(x, fa, at_ipa, at_pts, out);
    }
  }
  a.pre.res[node] = out;
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
// block_spread_mins is the block's walk (k_preempt_many_mins runs it too):
// over the present entries of d[0 .. V), those three in every thread (-1: no arg-min).
__device__ __forceinline__ void block_spread_mins(const int64_t* __restrict__ d, int32_t V, int64_t& m1, int32_t& v1,
                                                  int64_t& m2) {
  __shared__ int64_t sh_m[4];
  __shared__ int32_t sh_v[4];
  __shared__ int64_t s_m1;
  __shared__ int32_t s_v1;
  constexpr int64_t kNone = 2147483647;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // the pair (count, value id), smallest count first, then the smallest id
  auto less = [](int64_t ma, int32_t va, int64_t mb, int32_t vb) { return ma < mb || (ma == mb && va < vb); };
  m1 = kNone, m2 = kNone;
  v1 = -1;
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
}
__global__ __launch_bounds__(256) void k_preempt_spread_mins(DevCluster c, DevPods P,
                                                             const DevState* __restrict__ st, DevScratch s,
                                                             int64_t* __restrict__ smin, uint32_t hard) {
  int i = 0;                                           // this block's use
  for (int k = blockIdx.x; i < KSIM_MAX_USES; i++)
    if (((hard >> i) & 1u) && k-- == 0) break;
  if (i >= KSIM_MAX_USES) return;
  const int32_t pi = st->cursor;
  const ksim_pod& p = P.pods[pi];
  const ksim_topo_use u = load_use(P.uses + p.use_first, i);
  const int32_t V = u.col != KSIM_COL_NONE ? c.col_nvals[u.col] : 0;
  const int64_t* d = ((P.plans[pi].m.ptab >> i) & 1u) ? P.ptab + u._pad : s.dom + (size_t)i * c.vmax;
  int64_t m1, m2;
  int32_t v1;
  block_spread_mins(d, V, m1, v1, m2);
  if (threadIdx.x == 0) {
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

// ---- the batched dry run (ksim_preempt_many) --------------------------------------
// The node's TopoRow for the status step of a row whose plan reads no domain
// table: the filters left (NodePorts, the volume limit plugins) read the
// node's class counts of the uses in `read` and nothing else of the row, and
// neither the domain tables nor the topology flags (load_topo_row's node_count
// branch, entry for entry).
__device__ __forceinline__ void load_count_row(const DevCluster& c, const ksim_topo_use* U, int nu, uint32_t read,
                                               int32_t node, TopoRow& t) {
#pragma unroll
  for (int i = 0; i < KSIM_MAX_USES; i++) {
    t.v[i] = 0;
    t.x[i] = 0;
    if (i < nu && ((read >> i) & 1u)) t.x[i] = class_count(c, load_use(U, i).cls, node);
  }
}

// Per (node, row): the per-pod cycle's filter status of the row's preemptor on
// the node (run_filter_plan, the status pass's own function, the code kept in
// a register), then SelectVictimsOnNode as k_preempt_nodes runs it, on the
// row's own slabs, then the static veto.  Grid ((n + 255) / 256, rows).  The
// row record, its pod, plan and uses sit at block-uniform addresses: scalar
// loads.  VOL: the group's form is VolumeForm, else FreeForm or, behind one
// block-uniform branch, PortsForm.
template <bool VOL, bool PDB>
__global__ __launch_bounds__(256) void k_preempt_many_nodes(PreemptCommon a0, const PreemptRow* __restrict__ rows,
                                                            uint64_t rank_lo, uint64_t rank_hi) {
  const int32_t node = blockIdx.x * blockDim.x + threadIdx.x;
  // the node's row does not depend on the preemptor: its loads go out before the row record's chain
  const int32_t xr = node < a0.c.n ? node : a0.c.n - 1;
  const NodeRow r = load_row(a0.c, xr);
  const PreemptRow& row = rows[blockIdx.y];
  if (node >= a0.c.n) return;
  PreemptCommon a = a0;                                  // the row's view: its pod, slabs, priority and port uses
  a.P = row.P;
  a.pre.res = row.res;
  a.pre.vflag = row.vflag;
  a.prio = row.prio;
  a.port_mask = row.ports;
  const ksim_pod& p = a.P.pods[0];
  const PodPlan& pp = a.P.plans[0];
  const ksim_topo_use* U = a.P.uses + p.use_first;
  TopoRow t;
  load_count_row(a.c, U, p.use_count, pp.m.port | pp.m.vol, node, t);
  uint32_t det;
  const uint32_t f = run_filter_plan(a.c, a.P, FilterPlan{rank_lo, rank_hi, pp.filter_en}, nullptr, 0u, p, r, U, pp.m,
                                     t, det);
  PreemptNode out{};
  Trial x{a, p, pp, U, node, -1, 0, 0};
  bool at_ipa = false, at_pts = false;
  if constexpr (VOL) {
    if (VolumeForm::potential(f, a, row.vm, at_ipa, at_pts)) select_victims<VolumeForm, PDB>(x, row.vm, at_ipa, at_pts, out);
  } else {
    const PreemptDom none{};
    if (failed_fit_or_ports(f, a)) {
      if (a.port_mask)                                   // block-uniform
        select_victims<PortsForm, PDB>(x, none, at_ipa, at_pts, out);
      else
        select_victims<FreeForm, PDB>(x, none, at_ipa, at_pts, out);
    }
  }
  if ((row.vb | row.vz) && out.cand) {                   // k_preempt_static_veto's rule
    bool bad = false;
    if (row.vb && p.vb_count) bad = volume_binding_fails(a.c, a.P, p.vb_first, p.vb_count, node) != 0;
    if (!bad && row.vz && p.vz_count) bad = !volume_groups_match(a.c, a.P, p.vz_first, p.vz_count, node);
    if (bad) out.cand = 0;
  }
  row.res[node] = out;
}

// The nominated node's victims of every row, in the dry run's list order
// (preempt_read_back's): the rows flagged victim and violating, then the plain
// victims, each in CSR order, as indices into the caller's table (index).  One
// wave per row: it walks the node's range in the row's flag slab 64 rows at a
// time and compacts by ballot and a running count.  Nothing is written at or
// past the row's cap.
__global__ __launch_bounds__(64) void k_preempt_many_victims(const PreemptRow* __restrict__ rows,
                                                             const int32_t* __restrict__ pick,
                                                             const int32_t* __restrict__ off,
                                                             const int32_t* __restrict__ index) {
  const PreemptRow& row = rows[blockIdx.x];
  const int32_t node = pick[(size_t)blockIdx.x * kPickWords];
  if (node < 0 || row.cap <= 0) return;
  const int lane = threadIdx.x;
  const int32_t j0 = off[node], j1 = off[node + 1];
  int32_t k = 0;                                         // victims written so far (wave-uniform)
  for (int pass = 0; pass < 2; pass++) {
    const uint8_t want = pass == 0 ? (uint8_t)(1 | kPreemptViolating) : (uint8_t)1;
    for (int32_t base = j0; base < j1 && k < row.cap; base += 64) {
      const int32_t j = base + lane;
      const bool hit = j < j1 && row.vflag[j] == want;
      const uint64_t m = __ballot(hit);
      const int32_t at = k + (int32_t)__popcll(m & ((1ull << lane) - 1ull));
      if (hit && at < row.cap) row.victims[at] = index[j];
      k += (int32_t)__popcll(m);
    }
  }
}

// ---- the batched dry run's domain rows (ksim_preempt_many_dom) --------------------
// A row whose plan reads domain tables runs on a PreFilter state of its own
// (PreemptDomRow: tables in load_topo_row's indexing, and a head with the words
// a single dry run keeps per handle).  Four kernels per group, each on a grid
// with the row in blockIdx.y.
constexpr int kManyLdsDom = 128;   // tables of key columns with <= kManyLdsDom value ids are LDS-staged

// Before a group's PreFilter pass: what its rows read of their states is zero,
// whatever the group before left there.  Block (i, row) clears the entries of
// use i's table that load_topo_row can reach (the value ids of its key column)
// when the use has a table at all; block (0, row) also clears the head.  Grid
// (KSIM_MAX_USES, rows).
__global__ __launch_bounds__(256) void k_preempt_many_zero(DevCluster c, const PreemptRow* __restrict__ rows,
                                                           const PreemptDomRow* __restrict__ drows) {
  const int i = blockIdx.x;
  const PreemptDomRow& dr = drows[blockIdx.y];
  const DevPods& P = rows[blockIdx.y].P;
  if (i == 0) {
    int64_t* w = reinterpret_cast<int64_t*>(dr.head);
    for (int x = threadIdx.x; x < (int)(sizeof(PreemptDomHead) / 8); x += blockDim.x) w[x] = 0;
  }
  if (!((P.plans[0].m.dom >> i) & 1u)) return;              // block-uniform
  const int32_t V = c.col_nvals[load_use(P.uses + P.pods[0].use_first, i).col];
  int64_t* d = dr.dom + (size_t)i * c.vmax;
  for (int32_t v = threadIdx.x; v < V; v += blockDim.x) d[v] = 0;
}

// k_topo_prefilter's rule for the row's preemptor, for the uses a Filter reads
// (the status step never scores): per node, its class count into the entry of
// its value in every such table, a DoNotSchedule use's with the presence mark
// and only from the nodes PodTopologySpread counts (every hard key on the
// node, and the use's node inclusion policies); kTopoAffinityNonEmpty; and in
// the same pass k_preempt_totals' sums (afftot[i]: the class count over the
// nodes that carry the key, hostname-keyed uses included): a block sum in
// LDS, then one atomic per block and affinity use.  Integer atomics throughout, so the
// result does not depend on the order.  Grid ((n + 255) / 256, rows).
__global__ __launch_bounds__(256) void k_preempt_many_dom(DevCluster c, const PreemptRow* __restrict__ rows,
                                                          const PreemptDomRow* __restrict__ drows) {
  __shared__ unsigned long long s_dom[KSIM_MAX_USES][kManyLdsDom];
  __shared__ unsigned long long s_tot[KSIM_MAX_USES];
  __shared__ uint32_t s_flags;
  const PreemptDomRow& dr = drows[blockIdx.y];
  const DevPods& P = rows[blockIdx.y].P;           // block-uniform: scalar loads
  const ksim_pod& p = P.pods[0];
  const UseMasks& m = P.plans[0].m;
  const ksim_topo_use* U = P.uses + p.use_first;
  const uint32_t rd = m.hard | m.aff | m.anti | m.exist;   // the uses whose label and count the pass reads
  const uint32_t need = rd & m.dom;                         // ... and those with a table
  uint32_t lds = 0;                                         // uses whose table is staged in LDS
  for (uint32_t b = need; b; b &= b - 1) {
    const int i = __builtin_ctz(b);
    if (c.col_nvals[load_use(U, i).col] <= kManyLdsDom) lds |= 1u << i;
  }
  const int tid = threadIdx.x;
  for (int x = tid; x < KSIM_MAX_USES * kManyLdsDom; x += blockDim.x) s_dom[x / kManyLdsDom][x % kManyLdsDom] = 0;
  if (tid < KSIM_MAX_USES) s_tot[tid] = 0;
  if (tid == 0) s_flags = 0;
  __syncthreads();
  const int32_t node = blockIdx.x * blockDim.x + tid;
  uint32_t flags = 0;
  if (node < c.n) {
    uint32_t val[KSIM_MAX_USES];
    int64_t cnt[KSIM_MAX_USES];
#pragma unroll
    for (int i = 0; i < KSIM_MAX_USES; i++) {               // every load of the node first
      val[i] = 0;
      cnt[i] = 0;
      if ((rd >> i) & 1u) {
        const ksim_topo_use u = load_use(U, i);
        if (u.col != KSIM_COL_NONE) val[i] = c.labels[(size_t)u.col * c.n + node];
        cnt[i] = class_count(c, u.cls, node);
      }
    }
    bool all_hard = true;                                   // nodeLabelsMatchSpreadConstraints
#pragma unroll
    for (int i = 0; i < KSIM_MAX_USES; i++) {
      if (((m.hard >> i) & 1u) && val[i] == 0) all_hard = false;
      if (((m.aff >> i) & 1u) && val[i] != 0 && cnt[i] > 0) {
        flags |= kTopoAffinityNonEmpty;
        atomicAdd(&s_tot[i], (unsigned long long)cnt[i]);   // the block's sum, in LDS
      }
    }
    // matchNodeInclusionPolicies, once per node for every spread use
    const bool aff_ok = (m.honor_aff & m.hard) ? required_node_affinity_match(c, P, p, node) : true;
    const bool taint_ok = (m.honor_taints & m.hard) ? !node_has_untolerated_taint(c, p, node) : true;
#pragma unroll
    for (int i = 0; i < KSIM_MAX_USES; i++) {
      const uint32_t v = val[i];
      if (!((need >> i) & 1u) || v == 0) continue;          // no table, or the node has no pair for this key
      const bool incl = (!((m.honor_aff >> i) & 1u) || aff_ok) && (!((m.honor_taints >> i) & 1u) || taint_ok);
      int64_t add = cnt[i];
      if ((m.hard >> i) & 1u)                               // TpPairToMatchNum[pair] += count (+ presence mark)
        add = all_hard && incl ? add + (1ll << kDomMarkShift) : 0;
      if (add == 0) continue;
      if ((lds >> i) & 1u)
        atomicAdd(&s_dom[i][v], (unsigned long long)add);
      else
        atomicAdd(reinterpret_cast<unsigned long long*>(dr.dom + (size_t)i * c.vmax + v), (unsigned long long)add);
    }
  }
  if (flags) atomicOr(&s_flags, flags);
  __syncthreads();
  for (int x = tid; x < KSIM_MAX_USES * kManyLdsDom; x += blockDim.x) {
    if (!((lds >> (x / kManyLdsDom)) & 1u)) continue;
    const unsigned long long v = s_dom[x / kManyLdsDom][x % kManyLdsDom];
    if (v) atomicAdd(reinterpret_cast<unsigned long long*>(dr.dom + (size_t)(x / kManyLdsDom) * c.vmax + x % kManyLdsDom), v);
  }
  if (tid < KSIM_MAX_USES && s_tot[tid])
    atomicAdd(reinterpret_cast<unsigned long long*>(&dr.head->afftot[tid]), s_tot[tid]);
  if (tid == 0 && s_flags) atomicOr(&dr.head->topo_flags, s_flags);
}

// k_preempt_spread_mins over the row's own table: block (i, row) takes use i
// when it is a DoNotSchedule use of the row, and also leaves the minimum where
// the status step's pts_filter reads it (k_topo_min's word).  Grid
// (KSIM_MAX_USES, rows).
__global__ __launch_bounds__(256) void k_preempt_many_mins(DevCluster c, const PreemptRow* __restrict__ rows,
                                                           const PreemptDomRow* __restrict__ drows) {
  const int i = blockIdx.x;
  const PreemptDomRow& dr = drows[blockIdx.y];
  if (!((dr.hard >> i) & 1u)) return;                       // block-uniform
  const DevPods& P = rows[blockIdx.y].P;
  const ksim_topo_use u = load_use(P.uses + P.pods[0].use_first, i);
  const int32_t V = u.col != KSIM_COL_NONE ? c.col_nvals[u.col] : 0;
  int64_t m1, m2;
  int32_t v1;
  block_spread_mins(dr.dom + (size_t)i * c.vmax, V, m1, v1, m2);
  if (threadIdx.x == 0) {
    dr.head->smin[i][0] = m1;
    dr.head->smin[i][1] = v1;
    dr.head->smin[i][2] = m2;
    dr.head->min_match[i] = m1;
  }
}

// k_preempt_many_nodes for a group of rows with a row side: the status step
// reads the row's tables, minima and topology flags, and the trial state is
// RowForm<true> (hard may be empty: affinity alone) or FullForm, through the
// row's view of PreemptCommon (its tables and afftot swapped in beside its pod
// and slabs).  ipa_index / pts_index: PreemptDom's and PreemptSpread's.
template <class FORM, bool PDB>
__global__ __launch_bounds__(256) void k_preempt_many_dom_nodes(PreemptCommon a0, const PreemptRow* __restrict__ rows,
                                                                const PreemptDomRow* __restrict__ drows,
                                                                int32_t ipa_index, int32_t pts_index, uint64_t rank_lo,
                                                                uint64_t rank_hi) {
  const int32_t node = blockIdx.x * blockDim.x + threadIdx.x;
  const int32_t xr = node < a0.c.n ? node : a0.c.n - 1;
  const NodeRow r = load_row(a0.c, xr);
  const PreemptRow& row = rows[blockIdx.y];
  const PreemptDomRow& dr = drows[blockIdx.y];
  if (node >= a0.c.n) return;
  PreemptCommon a = a0;
  a.P = row.P;
  a.pre.res = row.res;
  a.pre.vflag = row.vflag;
  a.pre.afftot = dr.head->afftot;
  a.s.dom = dr.dom;
  a.s.min_match = dr.head->min_match;
  a.prio = row.prio;
  a.port_mask = row.ports;
  const ksim_pod& p = a.P.pods[0];
  const PodPlan& pp = a.P.plans[0];
  const ksim_topo_use* U = a.P.uses + p.use_first;
  uint32_t f;
  {
    TopoRow t;
    load_topo_row(a.c, U, p.use_count, pp.m, a.s, a.P.ptab, node, t);
    uint32_t det;
    f = run_filter_plan(a.c, a.P, FilterPlan{rank_lo, rank_hi, pp.filter_en}, a.s.min_match, dr.head->topo_flags, p, r,
                        U, pp.m, t, det);
  }
  PreemptNode out{};
  Trial x{a, p, pp, U, node, -1, 0, 0};
  bool at_ipa = false, at_pts = false;
  const PreemptSpread ds{{dr.aff, dr.anti, dr.exist, ipa_index}, dr.hard, pts_index, &dr.head->smin[0][0]};
  if constexpr (std::is_same_v<FORM, FullForm>) {
    const PreemptFull fa{ds, row.vm};
    if (FullForm::potential(f, a, fa, at_ipa, at_pts)) select_victims<FullForm, PDB>(x, fa, at_ipa, at_pts, out);
  } else {
    if (FORM::potential(f, a, ds, at_ipa, at_pts)) select_victims<FORM, PDB>(x, ds, at_ipa, at_pts, out);
  }
  if ((row.vb | row.vz) && out.cand) {                   // k_preempt_static_veto's rule
    bool bad = false;
    if (row.vb && p.vb_count) bad = volume_binding_fails(a.c, a.P, p.vb_first, p.vb_count, node) != 0;
    if (!bad && row.vz && p.vz_count) bad = !volume_groups_match(a.c, a.P, p.vz_first, p.vz_count, node);
    if (bad) out.cand = 0;
  }
  row.res[node] = out;
}

constexpr int kPickThreads = 1024;

// min_pct / min_abs: DefaultPreemptionArgs (calculateNumCandidates).  Block r
// scans the results at pre.res + r n and writes the record at pre.pick +
// r kPickWords (the batched dry run's rows; one block for a single dry run).
__global__ __launch_bounds__(kPickThreads) void k_preempt_pick(DevCluster c, DevPreempt pre, int32_t min_pct,
                                                               int32_t min_abs) {
  pre.res += (size_t)blockIdx.x * c.n;
  pre.pick += (size_t)blockIdx.x * kPickWords;
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

// ---- committed preemption (ksim_preempt_commit) -----------------------------------
// The victims of a dry run (or any list of deleted bound pods) leave the
// device's state: the snapshot as ksim_forget would leave it, and the bound
// table without their rows, the survivors in their order.  Six launches:
//   k_commit_begin    pos[caller's row] = position, dead[] = 0
//   k_commit_evict    one wave per victim: assume_pod_wave with sign -1, the
//                     attached volumes, dead[its position] = 1
//   k_commit_sums     per tile of kCommitTile positions: dead rows, and the
//                     surviving entries of each list set on the rows
//   k_commit_carry    one block: the exclusive scan of the tiles' sums
//   k_commit_scatter  per tile again: the scan inside the tile (per thread its
//                     kCommitTile / kCommitThreads consecutive rows, a wave64
//                     scan of the threads' sums by __shfl_up, the four waves'
//                     totals through LDS, the tile's carry), then every
//                     survivor's row and list entries into the second buffer
//                     set at position k - dead-before(k)
//   k_commit_off      off2[v] = off[v] - dead-before(off[v])
// The scatter goes to a second buffer set (shifting in place would overwrite
// rows a later thread still reads); the host swaps the handle's pointers.
// The carry between tiles is the three-launch reduce-then-scan, not a
// single-pass look-back: no block waits for another, so nothing depends on the
// dispatch order or on co-residency, and the tiles' sums of a million rows
// (977) are four passes of one block.  What the tiles read twice for it (a flag
// byte and the lists' offsets of every row) is small beside the 104 bytes a
// surviving row moves.
//
// Victims on one node: every column moves by a returnless atomic add, so the
// order of the waves does not matter.  The last-holder rule of volume_bind
// reads a class count before it moves it; here the move is a returning atomic
// add of -1 on the class count, and the one wave that gets 1 back took the
// last holding: it alone moves the family's distinct count.  The hardware
// serializes the adds on the word, whichever nodes and waves they come from.
__device__ __forceinline__ void volume_unbind_atomic(const DevCluster& c, const DevPods& P, const ksim_pod& p,
                                                     int32_t node) {
  if (!c.vol_nf) return;
  for (int i = 0; i < p.use_count; i++) {
    const ksim_topo_use u = P.uses[p.use_first + i];
    if (u.kind != KSIM_USE_VOLUME || (uint32_t)u._pad >= (uint32_t)c.vol_nf) continue;   // as volume_bind
    int32_t* att = c.vol_attached + (size_t)u._pad * c.n + node;
    if (u.cls < 0) {
      atomicAdd(att, -u.arg);
      continue;
    }
    if (atomicAdd(c.cnt + (size_t)u.cls * c.n + node, -1) == 1) atomicAdd(att, -1);
  }
}

__device__ __forceinline__ CommitSum operator+(const CommitSum& a, const CommitSum& b) {
  return CommitSum{a.dead + b.dead, a.adds + b.adds, a.pids + b.pids, a.vols + b.vols};
}
__device__ __forceinline__ CommitSum operator-(const CommitSum& a, const CommitSum& b) {
  return CommitSum{a.dead - b.dead, a.adds - b.adds, a.pids - b.pids, a.vols - b.vols};
}

// What position k adds to the scan: a dead row counts one, a survivor its
// lists' lengths, the end position (k == n) and everything past it nothing.
__device__ __forceinline__ CommitSum commit_row(const DevCommit& m, int32_t k) {
  CommitSum s{0, 0, 0, 0};
  if (k >= m.n) return s;
  if (m.dead[k]) {
    s.dead = 1;
    return s;
  }
  if (m.aoff) s.adds = m.aoff[k + 1] - m.aoff[k];
  if (m.poff) s.pids = m.poff[k + 1] - m.poff[k];
  if (m.voff) s.vols = m.voff[k + 1] - m.voff[k];
  return s;
}

// Exclusive scan of v over the block's kCommitThreads threads (every thread
// calls it); total: the block's sum.  s_wave: kCommitThreads / 64 LDS words.
__device__ __forceinline__ CommitSum commit_block_scan(const CommitSum& v, CommitSum* s_wave, CommitSum& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  CommitSum inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const CommitSum o{__shfl_up(inc.dead, d), __shfl_up(inc.adds, d), __shfl_up(inc.pids, d), __shfl_up(inc.vols, d)};
    if (lane >= d) inc = inc + o;
  }
  if (lane == 63) s_wave[w] = inc;
  __syncthreads();
  CommitSum base{0, 0, 0, 0};
  total = base;
#pragma unroll
  for (int x = 0; x < kCommitThreads / 64; x++) {
    const CommitSum t = s_wave[x];
    if (x < w) base = base + t;
    total = total + t;
  }
  __syncthreads();                                       // s_wave is free again
  return base + inc - v;
}

__global__ __launch_bounds__(256) void k_commit_begin(DevCommit m) {
  const int32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k > m.n) return;
  m.dead[k] = 0;
  if (k < m.n) m.pos[m.index[k]] = k;
}

__global__ __launch_bounds__(64) void k_commit_evict(DevCluster c, DevCommit m, const CommitRec* __restrict__ recs) {
  const CommitRec& r = recs[blockIdx.x];
  const ksim_pod& p = r.P.pods[0];
  assume_pod_wave(c, r.P, p, r.node, -1, true, nullptr, false);   // NodeInfo.RemovePod, the tables with it
  if (threadIdx.x == 7) volume_unbind_atomic(c, r.P, p, r.node);
  if (threadIdx.x == 63) m.dead[m.pos[r.row]] = 1;
}

// The sums of the thread's consecutive positions, and each one's own.
__device__ __forceinline__ CommitSum commit_thread_rows(const DevCommit& m, int32_t k0,
                                                        CommitSum (&r)[kCommitTile / kCommitThreads]) {
  CommitSum mine{0, 0, 0, 0};
#pragma unroll
  for (int q = 0; q < kCommitTile / kCommitThreads; q++) {
    r[q] = commit_row(m, k0 + q);
    mine = mine + r[q];
  }
  return mine;
}

__global__ __launch_bounds__(kCommitThreads) void k_commit_sums(DevCommit m) {
  __shared__ CommitSum s_wave[kCommitThreads / 64];
  CommitSum r[kCommitTile / kCommitThreads], total;
  const CommitSum mine =
      commit_thread_rows(m, blockIdx.x * kCommitTile + (int32_t)threadIdx.x * (kCommitTile / kCommitThreads), r);
  commit_block_scan(mine, s_wave, total);
  if (threadIdx.x == 0) m.tile[blockIdx.x] = total;
}

// tile[t] becomes the sums of the tiles before t: one block, kCommitThreads
// tiles a pass, the passes chained by a running carry.
__global__ __launch_bounds__(kCommitThreads) void k_commit_carry(DevCommit m, int32_t tiles) {
  __shared__ CommitSum s_wave[kCommitThreads / 64];
  CommitSum carry{0, 0, 0, 0};
  for (int32_t t0 = 0; t0 < tiles; t0 += kCommitThreads) {
    const int32_t t = t0 + (int32_t)threadIdx.x;
    const CommitSum v = t < tiles ? m.tile[t] : CommitSum{0, 0, 0, 0};
    CommitSum total;
    const CommitSum at = carry + commit_block_scan(v, s_wave, total);
    if (t < tiles) m.tile[t] = at;
    carry = carry + total;
  }
}

template <class E>
__device__ __forceinline__ void commit_list(const int32_t* off, const E* ent, int32_t* off2, E* ent2, int32_t k,
                                            int32_t k2, int32_t at, int32_t len) {
  if (!off) return;
  off2[k2] = at;                                         // (the end position: len = 0, the list's new length)
  const int32_t from = off[k];
  for (int32_t j = 0; j < len; j++) ent2[at + j] = ent[from + j];
}

__global__ __launch_bounds__(kCommitThreads) void k_commit_scatter(DevCommit m) {
  __shared__ CommitSum s_wave[kCommitThreads / 64];
  CommitSum r[kCommitTile / kCommitThreads], total;
  const int32_t k0 = blockIdx.x * kCommitTile + (int32_t)threadIdx.x * (kCommitTile / kCommitThreads);
  const CommitSum mine = commit_thread_rows(m, k0, r);
  CommitSum at = m.tile[blockIdx.x] + commit_block_scan(mine, s_wave, total);
#pragma unroll
  for (int q = 0; q < kCommitTile / kCommitThreads; q++) {
    const int32_t k = k0 + q;
    if (k > m.n) break;
    m.before[k] = at.dead;
    if (!r[q].dead) {                                    // a survivor, or the end position
      const int32_t k2 = k - at.dead;
      commit_list(m.aoff, m.adds, m.aoff2, m.adds2, k, k2, at.adds, r[q].adds);
      commit_list(m.poff, m.pids, m.poff2, m.pids2, k, k2, at.pids, r[q].pids);
      commit_list(m.voff, m.vols, m.voff2, m.vols2, k, k2, at.vols, r[q].vols);
      if (k < m.n) {
        m.prio2[k2] = m.prio[k];
        m.start2[k2] = m.start[k];
        m.index2[k2] = m.index[k];
#pragma unroll
        for (int x = 0; x < KSIM_PREEMPT_REQ; x++)
          m.req2[(size_t)k2 * KSIM_PREEMPT_REQ + x] = m.req[(size_t)k * KSIM_PREEMPT_REQ + x];
      }
    }
    at = at + r[q];
  }
}

__global__ __launch_bounds__(256) void k_commit_off(DevCommit m) {
  const int32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v > m.n_nodes) return;
  const int32_t o = m.off[v];
  m.off2[v] = o - m.before[o];
}

void launch_preempt_commit(const DevCluster& c, const DevCommit& m, const CommitRec* recs, int32_t n_victims,
                           hipStream_t stream) {
  const int32_t tiles = commit_tiles(m.n);
  k_commit_begin<<<m.n / 256 + 1, 256, 0, stream>>>(m);
  k_commit_evict<<<n_victims, 64, 0, stream>>>(c, m, recs);
  k_commit_sums<<<tiles, kCommitThreads, 0, stream>>>(m);
  k_commit_carry<<<1, kCommitThreads, 0, stream>>>(m, tiles);
  k_commit_scatter<<<tiles, kCommitThreads, 0, stream>>>(m);
  k_commit_off<<<m.n_nodes / 256 + 1, 256, 0, stream>>>(m);
}

template <class FORM>
static void launch_nodes(const PreemptCommon& ca, const typename FORM::Args& fa, hipStream_t stream) {
  auto nodes = ca.pre.poff != nullptr ? k_preempt_nodes<FORM, true> : k_preempt_nodes<FORM, false>;
  nodes<<<(ca.c.n + 255) / 256, 256, 0, stream>>>(ca, fa);
}

void launch_preempt(const LaunchArgs& a, const DevPreempt& pre, const PreemptPlan& q, hipStream_t stream) {
  const PreemptCommon ca{a.c, a.P, a.st, a.s, pre, q.fit, q.prio, q.port, q.ports};
  const PreemptFull fa{{{q.aff, q.anti, q.exist, q.ipa}, q.hard, q.pts, q.smin}, q.vol};
  // the form: by the uses the dry run reads (q.vol.voff: set for a preemptor with volume uses)
  const bool dom = q.reads_domains(), vol = q.vol.voff != nullptr;
  if (q.aff) k_preempt_totals<<<1, 256, 0, stream>>>(a.c, a.P, a.st, pre, q.aff);
  if (q.hard) k_preempt_spread_mins<<<__builtin_popcount(q.hard), 256, 0, stream>>>(a.c, a.P, a.st, a.s, q.smin, q.hard);
  if (vol && dom && q.vol.uses) launch_nodes<FullForm>(ca, fa, stream);
  else if (vol && !dom) launch_nodes<VolumeForm>(ca, fa.vm, stream);
  else if (q.hard) launch_nodes<SpreadForm>(ca, fa.ds, stream);
  else if (dom) launch_nodes<DomForm>(ca, fa.ds, stream);
  else launch_nodes<FreeForm>(ca, fa.ds, stream);
  if (q.vb || q.vz) k_preempt_static_veto<<<(a.c.n + 255) / 256, 256, 0, stream>>>(a.c, a.P, a.st, pre, q.vb, q.vz);
  k_preempt_pick<<<1, kPickThreads, 0, stream>>>(a.c, pre, a.prof.preempt_min_pct, a.prof.preempt_min_abs);
}

// The end of a launch group of either kind: every row's pick, then its victims list.
static void launch_many_picks(const LaunchArgs& a, const DevPreempt& pre, const PreemptMany& g, hipStream_t stream) {
  DevPreempt slabs = pre;                               // block r: the slab and the record of row r
  slabs.res = g.res;
  slabs.pick = g.pick;
  k_preempt_pick<<<g.n_rows, kPickThreads, 0, stream>>>(a.c, slabs, a.prof.preempt_min_pct, a.prof.preempt_min_abs);
  k_preempt_many_victims<<<g.n_rows, 64, 0, stream>>>(g.rows, g.pick, pre.off, g.index);
}

void launch_preempt_many(const LaunchArgs& a, const DevPreempt& pre, const PreemptPlan& q, const PreemptMany& g,
                         hipStream_t stream) {
  if (g.n_rows <= 0) return;
  // every row's own fields (its pod, slabs, priority, port uses) come from its record
  const PreemptCommon ca{a.c, DevPods{}, a.st, a.s, pre, q.fit, 0, q.port, 0u};
  const bool pdb = pre.poff != nullptr;
  auto nodes = g.volume ? (pdb ? k_preempt_many_nodes<true, true> : k_preempt_many_nodes<true, false>)
                        : (pdb ? k_preempt_many_nodes<false, true> : k_preempt_many_nodes<false, false>);
  nodes<<<dim3((a.c.n + 255) / 256, g.n_rows), 256, 0, stream>>>(ca, g.rows, g.rank_lo, g.rank_hi);
  launch_many_picks(a, pre, g, stream);
}

void launch_preempt_many_dom(const LaunchArgs& a, const DevPreempt& pre, const PreemptPlan& q, const PreemptMany& g,
                             const PreemptManyDom& d, hipStream_t stream) {
  if (g.n_rows <= 0) return;
  const PreemptCommon ca{a.c, DevPods{}, a.st, a.s, pre, q.fit, 0, q.port, 0u};
  const bool pdb = pre.poff != nullptr;
  const dim3 grid((a.c.n + 255) / 256, g.n_rows);
  k_preempt_many_zero<<<dim3(KSIM_MAX_USES, g.n_rows), 256, 0, stream>>>(a.c, g.rows, d.drows);
  k_preempt_many_dom<<<grid, 256, 0, stream>>>(a.c, g.rows, d.drows);
  if (d.spread) k_preempt_many_mins<<<dim3(KSIM_MAX_USES, g.n_rows), 256, 0, stream>>>(a.c, g.rows, d.drows);
  auto nodes = d.full ? (pdb ? k_preempt_many_dom_nodes<FullForm, true> : k_preempt_many_dom_nodes<FullForm, false>)
                      : (pdb ? k_preempt_many_dom_nodes<SpreadForm, true> : k_preempt_many_dom_nodes<SpreadForm, false>);
  nodes<<<grid, 256, 0, stream>>>(ca, g.rows, d.drows, q.ipa, q.pts, g.rank_lo, g.rank_hi);
  launch_many_picks(a, pre, g, stream);
}

}  // namespace ksim
