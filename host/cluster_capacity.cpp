// cluster_capacity — C++ mirror of the reference's main() (CC:48-150) over libkcc.
//
// Same flags, parsing, error exits and verdict text as
// src/KubeAPI/ClusterCapacity.go; the node/pod listing comes from a cluster file
// (-cluster) instead of client-go, and the two hot loops (CC:262-294, CC:105-140) run
// on the GPU through the C-ABI (kcc_capacity).  Additions: -specs <file> (a batch of
// what-if specs, one "cpuRequests memRequests replicas" per line), -v (per-node
// report of CC:107-117/137), -device/-gpus, -byPool (the totals per node pool, from
// the grouped fit: "Pool <name> : <total>" lines after the reference's output),
// -extRequests name=amount[,name=amount...] (the pod also requests extended resources —
// device-plugin GPUs, ephemeral-storage, hugepages — which the cluster file gives per node
// as `resource` lines and per container as `request` lines; in a -specs file trailing
// name=amount columns say the same per spec.  Totals, pools and -v's "Max replicas" then
// come from kcc_fit_ext; the output format does not change), and the opt-in spread
// constraints -maxPerNode k (at most k replicas on one node: required pod anti-affinity on the
// hostname), -spreadBy zone with -maxSkew k (default 1; topologySpreadConstraints over the
// cluster file's `zone` lines, DoNotSchedule).  They apply to every spec and compose with
// -byPool (the pools' totals under the per-node cap) and -extRequests; the totals then come
// from kcc_fit_capped and kcc_spread_fold, and with -spreadBy zone "Zone <name> : <used> of
// <cap>" lines follow the total.  Without them the output is the reference's.
// -deploy <file> (opt-in): a rollout plan placed on the nodes before every fit, one step per
// line, "cpuRequests memRequests replicas [pack|spread] [perNode:k] [name=amount ...]" ('#'
// comments as in a -specs file), in file order through kcc_deploy (consecutive lines of one
// policy share a call).  After the echo line (CC:85) each step prints "Deployed <cpu> <mem>
// <replicas> : <placed> on <nodes> nodes"; a step on which Go would panic prints the
// reference's panic line and exits with status 2.  Every later number — the total, -specs,
// -byPool, -maxPerNode, -spreadBy zone — then comes from the updated sums and pod counts.  -v
// with -deploy is refused (the verbose report recomputes its own sums).
// -explain (opt-in): under each spec's result, which resource binds the nodes and what is left
// over, from one ungrouped kcc_fit_explain call on the sums, -extRequests columns, -maxPerNode
// cap and post--deploy state of the total it explains: "Limited by <name> : <rows> nodes,
// <pods> replicas" per non-empty reason (cpu, memory, the extended resources by name, pods —
// the pod-slot clamp — and perNode — the cap), then "Left over <name> : <amount>" per resource
// (cpu in millicores with an m suffix).  Nothing for a spec on which Go would panic.  -explain
// with -spreadBy zone is refused: a maxSkew-clipped total is not a sum over rows.
// -priority p (opt-in): the preemption what-if.  The cluster file's `priority <int>` lines (after
// a `pod` line, default 0) split the pods in two levels: a pod of priority >= p stays, the rest
// make way.  Under each spec's result, "With preemption of pods below priority p : <total>, at
// most <V> pods evicted": the total from kcc_reduce_requests_levels + kcc_fit_levels (L = 2) on
// the plane without the lower-priority pods, V the pods below p on the rows.  An upper bound:
// every lower-priority pod yields (no PodDisruptionBudgets, no preemptionPolicy).  It composes
// with -extRequests, -maxPerNode, -specs and -byPool ("Pool <name> with preemption : <total>"
// lines after the pools'); with -schedulerRequests, -deploy and -spreadBy zone it is refused.
// -drain pool=<name> | zone=<name> | node=<a,b,...> (opt-in): the drain what-if.  The named
// nodes' rows go away; their pods (a pod's request is the sum of its app containers; a pod with
// a `daemon` line in the cluster file goes away with its node) are placed on the other nodes by
// kcc_drain, one step per distinct request shape, biggest first, under -drainPolicy pack|spread
// (default spread, the scheduler's least-allocated habit).  After the echo line (CC:85):
// "Drained <n> nodes : <E> pods evicted, <placed> placed, <U> not placed (<D> shapes)", or
// "..., shapes exceed <max>: none placed"; a shape with a zero cpu or memory request that meets
// free room is not placed and gets a "Drain shape <cpu>m <mem> : ..." line.  Every later number
// comes from the drained state.  A placement the scheduler could make, not the one it will:
// the evicted pods' selectors, affinities, PodDisruptionBudgets and priorities are not read.
// It composes with -specs, -byPool, -extRequests, -maxPerNode, -spreadBy zone and -explain;
// with -deploy, -priority, -schedulerRequests and -v it is refused.  A name no node carries is
// an error (exit status 1).  An unhealthy node among the named ones is not drained and not
// counted: its row is a zero row already (CC:221-226) and the reference lists no pods for it.
// -consolidate all | below=<pct> | node=<a,b,...> (opt-in): the removal what-if.  For each
// candidate node ON ITS OWN, its pods (requests and `daemon` pods as -drain's) are placed on the
// other nodes as they stand by kcc_consolidate, first fit in node order.  below=<pct>: the healthy
// nodes whose cpu AND memory request utilisation are both below pct per cent (used * 100 < pct *
// alloc, in integers: an autoscaler's scale-down threshold); an unhealthy node is never a
// candidate.  After the echo line (CC:85), one line per candidate in node order, "Node <name> :
// <e> pods evicted, <p> placed, <u> not placed, <z> without requests", then "Removable one at a
// time : <k> of <C> nodes (<k2> counting pods without requests as placed)".  A candidate with
// more than KCC_CONS_MAX_PODS evicted pods is not evaluated: its line is "Node <name> : <e> pods
// evicted, more than 1024: not evaluated", and it counts in <C> but never as removable.  The state is only
// read: every later number is what it is without the flag.  Nodes removable one at a time need
// not be removable together: -drain node=<those> is the joint check.  It composes with -specs,
// -byPool, -extRequests, -maxPerNode, -explain and -spreadBy zone; with -drain, -deploy,
// -priority, -schedulerRequests and -v it is refused.  A name no node carries is an error (exit
// status 1).
#include <array>
#include <cctype>
#include <cerrno>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "kcc.h"
#include "kcc_host.hpp"

using namespace kcchost;

namespace {

const char* kInvalidBytes =
    "byte quantity must be a positive integer with a unit of measurement like M, MB, MiB, G, "
    "GiB, or GB";
const char* kRule =
    "==============================================================================================================";

struct Flags {
  std::map<std::string, std::string> v = {
      {"kubeconfig", ""},         {"cluster", ""},          {"cpuRequests", "100m"},
      {"cpuLimits", "200m"},      {"memRequests", "100mb"}, {"memLimits", "200mb"},
      {"replicas", "1"},          {"specs", ""},            {"device", "0"},
      {"gpus", "1"},              {"v", "false"},           {"schedulerRequests", "false"},
      {"byPool", "false"},        {"extRequests", ""},      {"maxPerNode", "0"},
      {"spreadBy", ""},           {"maxSkew", "1"},         {"deploy", ""},
      {"explain", "false"},       {"priority", ""},         {"drain", ""},
      {"drainPolicy", "spread"}, {"consolidate", ""}};
};

// Go flag package syntax: -name=value, -name value, --name=value; bool -v.
bool parseFlags(int argc, char** argv, Flags& f) {
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    if (a.size() < 2 || a[0] != '-') {
      std::fprintf(stderr, "unexpected argument %s\n", a.c_str());
      return false;
    }
    a = a.substr(a[1] == '-' ? 2 : 1);
    std::string name = a, val;
    const size_t eq = a.find('=');
    bool has = false;
    if (eq != std::string::npos) {
      name = a.substr(0, eq);
      val = a.substr(eq + 1);
      has = true;
    }
    if (!f.v.count(name)) {
      std::fprintf(stderr, "flag provided but not defined: -%s\n", name.c_str());
      return false;
    }
    if ((name == "v" || name == "schedulerRequests" || name == "byPool" || name == "explain") &&
        !has) {
      val = "true";
    } else if (!has) {
      if (i + 1 >= argc) {
        std::fprintf(stderr, "flag needs an argument: -%s\n", name.c_str());
        return false;
      }
      val = argv[++i];
    }
    f.v[name] = val;
  }
  return true;
}

using NameAmount = std::vector<std::pair<std::string, std::string>>;
bool goAtoiStrict(const std::string& s, int64_t& out);

struct Spec {
  std::string cpuStr, memStr, repStr;
  uint64_t cpu = 0;
  int64_t mem = 0, replicas = 0;
  NameAmount ext;  // requests of extended resources (Quantity strings)
};

// "name=amount[,name=amount...]"; false on an item that is not name=amount.
bool parseExtList(const std::string& list, NameAmount& out) {
  std::istringstream is(list);
  std::string item;
  while (std::getline(is, item, ',')) {
    const size_t eq = item.find('=');
    if (eq == std::string::npos || eq == 0 || eq + 1 == item.size()) return false;
    out.emplace_back(item.substr(0, eq), item.substr(eq + 1));
  }
  return true;
}

// The spec lines of a -specs file as strings: "cpuRequests memRequests replicas" and any
// trailing name=amount columns (other trailing tokens are ignored, a '#' token ends them).
bool readSpecFile(const std::string& path, std::vector<Spec>& out) {
  std::ifstream sf(path);
  if (!sf) return false;
  std::string line;
  while (std::getline(sf, line)) {
    std::istringstream is(line);
    Spec s;
    if (!(is >> s.cpuStr >> s.memStr >> s.repStr) || s.cpuStr[0] == '#') continue;
    std::string tok;
    while (is >> tok && tok[0] != '#') {
      const size_t eq = tok.find('=');
      if (eq != std::string::npos && eq != 0) s.ext.emplace_back(tok.substr(0, eq), tok.substr(eq + 1));
    }
    out.push_back(s);
  }
  return true;
}

// One line of a -deploy file: a spec, the policy and the per-node cap (0: none).
struct Step {
  Spec spec;
  int policy = KCC_DEPLOY_PACK;
  int64_t perNode = 0;
};

// The steps of a -deploy file as strings.  0: read; 1: cannot open; 2: a token after the three
// columns that is neither pack, spread, perNode:<count> nor name=amount (bad holds it).
int readDeployFile(const std::string& path, std::vector<Step>& out, std::string& bad) {
  std::ifstream sf(path);
  if (!sf) return 1;
  std::string line;
  while (std::getline(sf, line)) {
    std::istringstream is(line);
    Step st;
    Spec& s = st.spec;
    if (!(is >> s.cpuStr >> s.memStr >> s.repStr) || s.cpuStr[0] == '#') continue;
    std::string tok;
    while (is >> tok && tok[0] != '#') {
      const size_t eq = tok.find('=');
      if (tok == "pack") {
        st.policy = KCC_DEPLOY_PACK;
      } else if (tok == "spread") {
        st.policy = KCC_DEPLOY_SPREAD;
      } else if (tok.compare(0, 8, "perNode:") == 0) {
        if (!goAtoiStrict(tok.substr(8), st.perNode) || st.perNode < 0) {
          bad = tok;
          return 2;
        }
      } else if (eq != std::string::npos && eq != 0 && eq + 1 != tok.size()) {
        s.ext.emplace_back(tok.substr(0, eq), tok.substr(eq + 1));
      } else {
        bad = tok;
        return 2;
      }
    }
    out.push_back(st);
  }
  return 0;
}

// The extended resources of a run: the union of the names the specs request, in
// first-appearance order, and every amount as Quantity.Value().
struct ExtRun {
  std::vector<std::string> names;
  std::vector<int64_t> spec_x;   // [R * S]
  std::vector<int64_t> alloc_x;  // [R * N]; a node without a `resource` line of a name: 0
  std::vector<int64_t> used_x;   // [R * N]
  std::map<const Container*, std::array<int64_t, KCC_EXT_MAX>> creq;  // per app container
  int64_t R() const { return (int64_t)names.size(); }
  int index(const std::string& name) const {
    for (size_t r = 0; r < names.size(); ++r)
      if (names[r] == name) return (int)r;
    return -1;
  }
};

// Names from the specs (more than KCC_EXT_MAX: an error), then every amount of the run —
// the specs' requests, the nodes' `resource` lines, the containers' `request` lines of
// those names — in one kcc_parse_quantity batch.  Returns false with a message.
bool loadExt(kcc_ctx* ctx, const std::vector<Spec>& specs, const Cluster& cl, ExtRun& x,
             std::string& err) {
  for (const Spec& s : specs)
    for (const auto& na : s.ext)
      if (x.index(na.first) < 0) x.names.push_back(na.first);
  if (x.R() > KCC_EXT_MAX) {
    err = "too many extended resources: " + std::to_string(x.R()) + " names requested, at most " +
          std::to_string(KCC_EXT_MAX);
    return false;
  }
  const size_t R = (size_t)x.R(), S = specs.size(), N = cl.nodes.size();
  x.spec_x.assign(R * S, 0);
  x.alloc_x.assign(R * N, 0);
  std::string chars;
  std::vector<int64_t> off{0};
  std::vector<int64_t*> dst;                       // where each parsed value goes
  std::vector<std::pair<const std::string*, const std::string*>> what;  // (name, amount)
  auto add = [&](const std::pair<std::string, std::string>& na, int64_t* to) {
    chars += na.second;
    off.push_back((int64_t)chars.size());
    dst.push_back(to);
    what.emplace_back(&na.first, &na.second);
  };
  for (size_t s = 0; s < S; ++s)
    for (const auto& na : specs[s].ext) add(na, &x.spec_x[(size_t)x.index(na.first) * S + s]);
  for (size_t i = 0; i < N; ++i)
    for (const auto& na : cl.nodes[i].resources)
      if (x.index(na.first) >= 0) add(na, &x.alloc_x[(size_t)x.index(na.first) * N + i]);
  for (const Pod& p : cl.pods)
    for (const Container& ct : p.containers) {
      if (ct.init) continue;  // requests of init containers are not read
      for (const auto& na : ct.requests)
        if (x.index(na.first) >= 0) {
          auto it = x.creq.emplace(&ct, std::array<int64_t, KCC_EXT_MAX>{}).first;
          add(na, &it->second[(size_t)x.index(na.first)]);
        }
    }
  const int64_t ns = (int64_t)dst.size();
  std::vector<int64_t> val((size_t)ns);
  std::vector<int8_t> st((size_t)ns);
  chars.resize((chars.size() + 4) & ~(size_t)3, '\0');  // 4-byte padded buffer
  if (ns > 0) {
    const int rc = kcc_parse_quantity(ctx, ns, chars.data(), off[(size_t)ns], off.data(), val.data(),
                                      st.data());
    if (rc) {
      err = std::string("kcc error ") + std::to_string(rc) + ": " + kcc_last_error(ctx);
      return false;
    }
  }
  for (int64_t k = 0; k < ns; ++k) {
    if (st[(size_t)k] != KCC_PARSE_OK) {
      err = "invalid quantity \"" + *what[(size_t)k].second + "\" for resource " +
            *what[(size_t)k].first;
      return false;
    }
    *dst[(size_t)k] = val[(size_t)k];
  }
  return true;
}

// Per-node sums of the containers' requests of each resource (the memory column's wrapping
// int64 sum, CC:291/293) through kcc_reduce_requests: a resource's per-container column
// rides in an int64 slot (mem_req / mem_lim), two resources per call.  Unhealthy nodes' zero
// rows get 0 allocatable.
int sumExt(kcc_ctx* ctx, const std::vector<node>& rows, const EngineInputs& in, ExtRun& x) {
  const size_t R = (size_t)x.R(), n = rows.size(), nc = in.app.size();
  for (size_t i = 0; i < n; ++i)
    if (rows[i].name.empty())
      for (size_t r = 0; r < R; ++r) x.alloc_x[r * n + i] = 0;
  x.used_x.assign(R * n, 0);
  if (n == 0 || nc == 0) return KCC_OK;
  std::vector<uint64_t> cpu_out(n), cpu_out2(n);
  std::vector<int64_t> col[2], out[2];
  for (size_t r0 = 0; r0 < R; r0 += 2) {
    for (size_t j = 0; j < 2; ++j) {
      col[j].assign(nc, 0);
      out[j].assign(n, 0);
      if (r0 + j >= R) continue;
      for (size_t k = 0; k < nc; ++k) {
        const auto it = x.creq.find(in.app[k]);
        if (it != x.creq.end()) col[j][k] = it->second[r0 + j];
      }
    }
    const int rc = kcc_reduce_requests(ctx, (int64_t)n, (int64_t)nc, in.node_ptr.data(),
                                       in.cpu_req.data(), col[0].data(), in.cpu_lim.data(),
                                       col[1].data(), cpu_out.data(), out[0].data(),
                                       cpu_out2.data(), out[1].data());
    if (rc) return rc;
    for (size_t j = 0; j < 2 && r0 + j < R; ++j)
      std::copy(out[j].begin(), out[j].end(), x.used_x.begin() + (long)((r0 + j) * n));
  }
  return KCC_OK;
}

bool goAtoiStrict(const std::string& s, int64_t& out) {
  char* end = nullptr;
  errno = 0;
  if (s.empty()) return false;
  const long long v = std::strtoll(s.c_str(), &end, 10);
  if (errno || *end || std::isspace((unsigned char)s[0])) return false;
  out = v;
  return true;
}

// CC:64-83: parse one spec exactly like the flags; exits like the reference on error.
// Go fmt "%.2f" (CC:117): NaN prints "NaN" and infinities "+Inf" / "-Inf" (an
// unhealthy node's zero row divides 0 by 0, CC:112-115); finite values format like C's.
std::string goF2(double x) {
  if (std::isnan(x)) return "NaN";
  if (std::isinf(x)) return x > 0 ? "+Inf" : "-Inf";
  char b[64];
  std::snprintf(b, sizeof b, "%.2f", x);
  return b;
}

void parseSpec(Spec& s, bool verbose_errors) {
  s.cpu = convertCPUToMilis(s.cpuStr);
  const auto mem = ToBytes(s.memStr);
  if (!mem.second) {
    std::printf("ERROR : Invalid input memRequests = %" PRId64 " %s ...exiting\n", mem.first,
                kInvalidBytes);
    std::exit(1);
  }
  s.mem = mem.first;
  if (!goAtoiStrict(s.repStr, s.replicas)) {
    std::printf("ERROR : Invalid input replicas = 0 strconv.Atoi: parsing \"%s\": invalid syntax "
                "...exiting\n", s.repStr.c_str());
    std::exit(1);
  }
  (void)verbose_errors;
}

int fail(kcc_ctx* ctx, int rc) {
  std::fprintf(stderr, "kcc error %d: %s\n", rc, ctx ? kcc_last_error(ctx) : kcc_create_error());
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  Flags f;
  if (!parseFlags(argc, argv, f)) return 2;
  const bool verbose = f.v["v"] == "true";
  // opt-in (NOT the reference's semantics): pod requests as the
  // scheduler counts them — init containers, sidecars, overhead
  const bool schedReq = f.v["schedulerRequests"] == "true";
  // the totals per node pool (the cluster file's `pool` lines) after the reference's output
  const bool byPool = f.v["byPool"] == "true";

  // opt-in spread constraints (NOT the reference's arithmetic)
  int64_t maxPerNode = 0, maxSkew = 1;
  if (!goAtoiStrict(f.v["maxPerNode"], maxPerNode) || maxPerNode < 0) {
    std::fprintf(stderr, "invalid value \"%s\" for flag -maxPerNode: want a count (0: no cap)\n",
                 f.v["maxPerNode"].c_str());
    return 2;
  }
  if (!goAtoiStrict(f.v["maxSkew"], maxSkew) || maxSkew < 1) {
    std::fprintf(stderr, "invalid value \"%s\" for flag -maxSkew: want a count of at least 1\n",
                 f.v["maxSkew"].c_str());
    return 2;
  }
  if (!f.v["spreadBy"].empty() && f.v["spreadBy"] != "zone") {
    std::fprintf(stderr, "invalid value \"%s\" for flag -spreadBy: want zone\n",
                 f.v["spreadBy"].c_str());
    return 2;
  }
  const bool byZone = f.v["spreadBy"] == "zone";
  const bool spread = byZone || maxPerNode > 0;
  // opt-in explanation of the total (NOT the reference's arithmetic)
  const bool explain = f.v["explain"] == "true";
  if (explain && byZone) {
    std::fprintf(stderr, "-explain cannot be combined with -spreadBy zone: a total clipped by maxSkew is not a sum over the nodes\n");
    return 2;
  }

  // opt-in rollout plan (NOT the reference's arithmetic): its steps as strings
  const bool deployOn = !f.v["deploy"].empty();
  // opt-in preemption what-if (NOT the reference's arithmetic)
  const bool prioOn = !f.v["priority"].empty();
  int64_t prio = 0;
  if (prioOn) {
    if (!goAtoiStrict(f.v["priority"], prio)) {
      std::fprintf(stderr, "invalid value \"%s\" for flag -priority: want an integer priority\n",
                   f.v["priority"].c_str());
      return 2;
    }
    const char* with = schedReq ? "-schedulerRequests" : deployOn ? "-deploy" : byZone ? "-spreadBy zone" : nullptr;
    if (with) {
      std::fprintf(stderr, "-priority cannot be combined with %s: the per-priority sums are the app-container sums of the pods as they stand, and a total clipped by maxSkew has no per-level form\n", with);
      return 2;
    }
  }
  // opt-in drain what-if (NOT the reference's arithmetic): which rows go away, and the policy
  // under which their pods are placed on the rest
  const bool drainOn = !f.v["drain"].empty();
  std::string drainKind;
  std::vector<std::string> drainNames;
  int drainPolicy = KCC_DEPLOY_SPREAD;
  if (f.v["drainPolicy"] == "pack") {
    drainPolicy = KCC_DEPLOY_PACK;
  } else if (f.v["drainPolicy"] != "spread") {
    std::fprintf(stderr, "invalid value \"%s\" for flag -drainPolicy: want pack or spread\n",
                 f.v["drainPolicy"].c_str());
    return 2;
  }
  if (drainOn) {
    const std::string& d = f.v["drain"];
    const size_t eq = d.find('=');
    drainKind = eq == std::string::npos ? "" : d.substr(0, eq);
    if ((drainKind != "pool" && drainKind != "zone" && drainKind != "node") || eq + 1 == d.size()) {
      std::fprintf(stderr, "invalid value \"%s\" for flag -drain: want pool=<name>, zone=<name> or node=<a,b,...>\n",
                   d.c_str());
      return 2;
    }
    if (drainKind == "node") {
      std::istringstream is(d.substr(eq + 1));
      std::string item;
      while (std::getline(is, item, ','))
        if (!item.empty()) drainNames.push_back(item);
    } else {
      drainNames.push_back(d.substr(eq + 1));
    }
    if (drainNames.empty()) {  // node=, : no name at all
      std::fprintf(stderr, "invalid value \"%s\" for flag -drain: want pool=<name>, zone=<name> or node=<a,b,...>\n",
                   d.c_str());
      return 2;
    }
    const char* with = deployOn ? "-deploy" : prioOn ? "-priority" : schedReq ? "-schedulerRequests" : verbose ? "-v" : nullptr;
    if (with) {
      std::fprintf(stderr, "-drain cannot be combined with %s: the drain places the evicted pods' app-container sums on the per-node sums as they stand, in one pass of its own\n", with);
      return 2;
    }
  }
  // opt-in removal what-if (NOT the reference's arithmetic): the candidate nodes
  const bool consOn = !f.v["consolidate"].empty();
  std::string consKind;  // all, below or node
  std::vector<std::string> consNames;
  int64_t consPct = 0;
  if (consOn) {
    const std::string& d = f.v["consolidate"];
    const size_t eq = d.find('=');
    consKind = eq == std::string::npos ? d : d.substr(0, eq);
    bool ok = (consKind == "all" && eq == std::string::npos) ||
              ((consKind == "below" || consKind == "node") && eq != std::string::npos && eq + 1 < d.size());
    if (ok && consKind == "below") {
      const std::string v = d.substr(eq + 1);
      ok = v.size() <= 9 && v.find_first_not_of("0123456789") == std::string::npos;
      if (ok) consPct = std::atoll(v.c_str());
    }
    if (ok && consKind == "node") {
      std::istringstream is(d.substr(eq + 1));
      std::string item;
      while (std::getline(is, item, ','))
        if (!item.empty()) consNames.push_back(item);
      ok = !consNames.empty();
    }
    if (!ok) {
      std::fprintf(stderr, "invalid value \"%s\" for flag -consolidate: want all, below=<pct> or node=<a,b,...>\n",
                   d.c_str());
      return 2;
    }
    const char* with = drainOn ? "-drain" : deployOn ? "-deploy" : prioOn ? "-priority" : schedReq ? "-schedulerRequests" : verbose ? "-v" : nullptr;
    if (with) {
      std::fprintf(stderr, "-consolidate cannot be combined with %s: each candidate's pods are placed on the per-node app-container sums as they stand, and the state is left alone\n", with);
      return 2;
    }
  }
  std::vector<Step> plan;
  if (deployOn) {
    if (verbose) {
      std::fprintf(stderr, "-v cannot be combined with -deploy: the per-node report recomputes its own sums\n");
      return 2;
    }
    std::string bad;
    const int drc = readDeployFile(f.v["deploy"], plan, bad);
    if (drc == 1) {
      std::fprintf(stderr, "cannot open deploy file %s\n", f.v["deploy"].c_str());
      return 1;
    }
    if (drc == 2) {
      std::fprintf(stderr, "invalid token \"%s\" in deploy file %s: want pack, spread, perNode:<count> or name=amount\n",
                   bad.c_str(), f.v["deploy"].c_str());
      return 2;
    }
  }

  Spec one{f.v["cpuRequests"], f.v["memRequests"], f.v["replicas"], 0, 0, 0, {}};
  if (!parseExtList(f.v["extRequests"], one.ext)) {
    std::fprintf(stderr, "invalid value \"%s\" for flag -extRequests: want name=amount[,name=amount...]\n",
                 f.v["extRequests"].c_str());
    return 2;
  }
  // the spec lines as strings; they are parsed where the reference parses its flags (below)
  std::vector<Spec> specs;
  const bool specFileOk = f.v["specs"].empty() || readSpecFile(f.v["specs"], specs);
  if (f.v["specs"].empty()) specs.push_back(one);

  // Extended resources: when a spec names one, the cluster is loaded and every amount
  // converted before anything is printed — a rejected quantity or a fifth name is a load
  // error (stderr, exit status 1, nothing on stdout).
  Cluster cl;
  kcc_ctx* ctx = nullptr;
  ExtRun ext;
  bool useExt = false;
  for (const Spec& s : specs) useExt = useExt || !s.ext.empty();
  // the plan's resource names count towards KCC_EXT_MAX with the specs': one name list, the
  // specs' columns first (ext.spec_x [R * S]), then the steps' (plan_x [R * K])
  std::vector<Spec> named(specs);
  for (const Step& st : plan) {
    useExt = useExt || !st.spec.ext.empty();
    named.push_back(st.spec);
  }
  std::vector<int64_t> plan_x;
  const std::string path = !f.v["cluster"].empty() ? f.v["cluster"] : f.v["kubeconfig"];
  if (useExt) {
    std::string err;
    if (path.empty()) {
      std::fprintf(stderr, "no cluster: pass -cluster <file> (client-go is not part of this build)\n");
      return 1;
    }
    if (!loadCluster(path, cl, err)) {
      std::fprintf(stderr, "panic: %s\n", err.c_str());
      return 2;
    }
    const int rc = kcc_create(&ctx, std::atoi(f.v["device"].c_str()), std::atoi(f.v["gpus"].c_str()));
    if (rc) return fail(nullptr, rc);
    if (!loadExt(ctx, named, cl, ext, err)) {
      std::fprintf(stderr, "%s\n", err.c_str());
      kcc_destroy(ctx);
      return 1;
    }
    if (deployOn) {  // split the columns: the specs', the steps'
      const size_t R = (size_t)ext.R(), S0 = specs.size(), K = plan.size();
      const std::vector<int64_t> all(ext.spec_x);
      ext.spec_x.assign(R * S0, 0);
      plan_x.assign(R * K, 0);
      for (size_t r = 0; r < R; ++r) {
        for (size_t s = 0; s < S0; ++s) ext.spec_x[r * S0 + s] = all[r * (S0 + K) + s];
        for (size_t k = 0; k < K; ++k) plan_x[r * K + k] = all[r * (S0 + K) + S0 + k];
      }
    }
  }
  const uint64_t cpuLimits = convertCPUToMilis(f.v["cpuLimits"]);            // CC:65
  parseSpec(one, true);                                                      // CC:64, 67-71, 79-83
  const auto memLim = ToBytes(f.v["memLimits"]);                             // CC:73-77
  if (!memLim.second) {
    std::printf("ERROR : Invalid input memLimits = %" PRId64 " %s ...exiting\n", memLim.first,
                kInvalidBytes);
    return 1;
  }
  std::printf("\nCPU limits, requests, Memory limits, requests and replicas parsed from input : "
              "%" PRIu64 " %" PRIu64 " %" PRId64 " %" PRId64 " %" PRId64 "\n",
              cpuLimits, one.cpu, memLim.first, one.mem, one.replicas);  // CC:85

  if (!f.v["specs"].empty()) {
    if (!specFileOk) {
      std::fprintf(stderr, "cannot open spec file %s\n", f.v["specs"].c_str());
      return 1;
    }
    for (Spec& s : specs) parseSpec(s, false);
  } else {
    specs[0] = one;  // (parsed above, CC:64-83)
  }
  for (Step& st : plan) parseSpec(st.spec, false);

  // cluster access (CC:88-99): a cluster file replaces kubeconfig + client-go
  if (path.empty()) {
    std::fprintf(stderr, "no cluster: pass -cluster <file> (client-go is not part of this build)\n");
    return 1;
  }
  int rc = 0;
  if (!useExt) {  // (with extended resources: loaded and created above)
    std::string err;
    if (!loadCluster(path, cl, err)) {
      std::fprintf(stderr, "panic: %s\n", err.c_str());
      return 2;
    }
    rc = kcc_create(&ctx, std::atoi(f.v["device"].c_str()), std::atoi(f.v["gpus"].c_str()));
    if (rc) return fail(nullptr, rc);
  }
  std::vector<node> rows;
  rc = getHealthyNodes(ctx, cl, rows);  // node cpu / memory strings parsed on the device
  if (rc) return fail(ctx, rc);
  EngineInputs in;
  rc = buildInputs(ctx, cl, rows, in);  // container cpu strings parsed on the device
  if (rc) return fail(ctx, rc);
  const int64_t n = (int64_t)rows.size(), nc = (int64_t)in.cpu_req.size();

  // -schedulerRequests: the per-node request sums of the opt-in model, fed to the fit
  std::vector<uint64_t> suc;
  std::vector<int64_t> sum_;
  if (schedReq) {
    suc.resize((size_t)n);
    sum_.resize((size_t)n);
    const int64_t np = (int64_t)in.ovh_cpu.size(), ni = (int64_t)in.init_mem.size();
    rc = kcc_reduce_requests_pods(ctx, n, np, nc, ni, in.node_pod_ptr.data(), in.pod_ptr.data(),
                                  in.cpu_req.data(), in.mem_req.data(), in.init_ptr.data(),
                                  ni ? in.init_cpu.data() : nullptr,
                                  ni ? in.init_mem.data() : nullptr,
                                  ni ? in.init_rst.data() : nullptr,
                                  np ? in.ovh_cpu.data() : nullptr,
                                  np ? in.ovh_mem.data() : nullptr, suc.data(), sum_.data());
    if (rc) return fail(ctx, rc);
  }

  // extended resources: the per-node sums of each, and the cpu / memory sums kcc_fit_ext takes
  std::vector<uint64_t> euc(suc);
  std::vector<int64_t> eum(sum_);
  if (useExt) {
    rc = sumExt(ctx, rows, in, ext);
    if (rc) return fail(ctx, rc);
    if (!schedReq) {
      euc.assign((size_t)n, 0);
      eum.assign((size_t)n, 0);
      rc = kcc_reduce_requests(ctx, n, nc, in.node_ptr.data(), in.cpu_req.data(), in.mem_req.data(),
                               nullptr, nullptr, euc.data(), eum.data(), nullptr, nullptr);
      if (rc) return fail(ctx, rc);
    }
  }
  const int64_t S = (int64_t)specs.size();

  // -deploy: the plan's steps on the per-node sums and pod counts, in file order; every fit
  // below then reads the updated state (suc / sum_ / euc / eum, in.pod_count, ext.used_x) as
  // the -schedulerRequests path reads its explicit sums
  const bool explicitSums = schedReq || deployOn || drainOn;
  if (deployOn) {
    if (!schedReq && !useExt) {  // the per-node request sums (CC:290-293)
      euc.assign((size_t)n, 0);
      eum.assign((size_t)n, 0);
      rc = kcc_reduce_requests(ctx, n, nc, in.node_ptr.data(), in.cpu_req.data(), in.mem_req.data(),
                               nullptr, nullptr, euc.data(), eum.data(), nullptr, nullptr);
      if (rc) return fail(ctx, rc);
    }
    const size_t K = plan.size(), R = (size_t)ext.R();
    for (size_t k0 = 0; k0 < K;) {
      size_t k1 = k0 + 1;
      while (k1 < K && plan[k1].policy == plan[k0].policy) ++k1;
      const size_t kn = k1 - k0;
      std::vector<uint64_t> pc(kn);
      std::vector<int64_t> pm(kn), prep(kn), pcap(kn), px(R * kn), placed(kn), used(kn);
      std::vector<int32_t> perr(kn);
      for (size_t k = 0; k < kn; ++k) {
        const Step& st = plan[k0 + k];
        pc[k] = st.spec.cpu;
        pm[k] = st.spec.mem;
        prep[k] = st.spec.replicas;
        pcap[k] = st.perNode;
        for (size_t r = 0; r < R; ++r) px[r * kn + k] = plan_x[r * K + k0 + k];
      }
      rc = kcc_deploy(ctx, n, in.alloc_cpu.data(), in.alloc_mem.data(), in.alloc_pods.data(),
                      ext.R(), ext.alloc_x.data(), in.pod_count.data(), euc.data(), eum.data(),
                      ext.used_x.data(), nullptr, 1, nullptr, (int64_t)kn, pc.data(), pm.data(),
                      px.data(), prep.data(), pcap.data(), plan[k0].policy, placed.data(),
                      used.data(), perr.data(), nullptr);
      if (rc) return fail(ctx, rc);
      for (size_t k = 0; k < kn; ++k) {
        const Spec& s = plan[k0 + k].spec;
        if (perr[k]) {
          std::fprintf(stderr, "panic: runtime error: integer divide by zero\n");
          kcc_destroy(ctx);
          return 2;
        }
        std::printf("Deployed %s %s %s : %" PRId64 " on %" PRId64 " nodes\n", s.cpuStr.c_str(),
                    s.memStr.c_str(), s.repStr.c_str(), placed[k], used[k]);
      }
      k0 = k1;
    }
    suc = euc;
    sum_ = eum;
  }

  // -drain and -consolidate: every counted pod's request (the sum of its app containers,
  // CC:276-294; px [R * P] from the -extRequests columns) and whether it can move (no `daemon`
  // line)
  const auto podRequests = [&](std::vector<uint64_t>& pcpu, std::vector<int64_t>& pmem,
                               std::vector<int64_t>& px, std::vector<uint8_t>& movable) {
    const size_t P = in.pod_daemon.size(), R = (size_t)ext.R();
    pcpu.assign(P, 0);
    pmem.assign(P, 0);
    px.assign(R * P, 0);
    movable.resize(P);
    for (size_t p = 0; p < P; ++p) {
      movable[p] = in.pod_daemon[p] ? 0 : 1;
      for (int64_t k = in.lv_pod_ptr[p]; k < in.lv_pod_ptr[p + 1]; ++k) {
        pcpu[p] += in.cpu_req[(size_t)k];
        pmem[p] = (int64_t)((uint64_t)pmem[p] + (uint64_t)in.mem_req[(size_t)k]);
        const auto it = ext.creq.find(in.app[(size_t)k]);
        if (it == ext.creq.end()) continue;
        for (size_t r = 0; r < R; ++r)
          px[r * P + p] = (int64_t)((uint64_t)px[r * P + p] + (uint64_t)it->second[r]);
      }
    }
  };

  // -drain: the rows of the named pool, zone or nodes go away.  Row i is node i's; a pod's
  // request is the sum of its app containers (CC:276-294), a `daemon` pod goes away with its
  // node.  kcc_drain leaves the drained rows full and places the evicted pods on the rest;
  // every fit below reads the updated state, as after -deploy.
  if (drainOn) {
    std::vector<uint8_t> mask((size_t)n, 0);
    for (const std::string& want : drainNames) {
      bool found = false;
      for (int64_t i = 0; i < n; ++i) {
        const NodeObj& nd = cl.nodes[(size_t)i];
        const std::string& have = drainKind == "pool" ? nd.pool : drainKind == "zone" ? nd.zone : nd.name;
        if (have == want) {
          // an unhealthy node's row is a zero row already (CC:221-226) and the reference lists
          // no pods for it: the name is known, but there is nothing to drain and it is not counted
          if (!rows[(size_t)i].name.empty()) mask[(size_t)i] = 1;
          found = true;
        }
      }
      if (!found) {
        std::fprintf(stderr, "-drain: no node with %s %s in %s\n", drainKind == "node" ? "name" : drainKind.c_str(),
                     want.c_str(), path.c_str());
        kcc_destroy(ctx);
        return 1;
      }
    }
    if (!useExt) {  // the per-node request sums (CC:290-293)
      euc.assign((size_t)n, 0);
      eum.assign((size_t)n, 0);
      rc = kcc_reduce_requests(ctx, n, nc, in.node_ptr.data(), in.cpu_req.data(), in.mem_req.data(),
                               nullptr, nullptr, euc.data(), eum.data(), nullptr, nullptr);
      if (rc) return fail(ctx, rc);
    }
    const size_t P = in.pod_daemon.size(), R = (size_t)ext.R();
    std::vector<uint64_t> pcpu;
    std::vector<int64_t> pmem, px;
    std::vector<uint8_t> movable;
    podRequests(pcpu, pmem, px, movable);
    const int64_t M = KCC_DRAIN_MAX_SHAPES;
    int64_t summary[KCC_DRAIN_SUMMARY] = {0, 0, 0, 0};
    std::vector<uint64_t> shc((size_t)M);
    std::vector<int64_t> shm((size_t)M), shx(R * (size_t)M), shn((size_t)M), shp((size_t)M), shu((size_t)M);
    std::vector<int32_t> she((size_t)M);
    rc = kcc_drain(ctx, n, in.alloc_cpu.data(), in.alloc_mem.data(), in.alloc_pods.data(), ext.R(),
                   ext.alloc_x.data(), in.pod_count.data(), euc.data(), eum.data(), ext.used_x.data(),
                   mask.data(), (int64_t)P, in.lv_node_pod_ptr.data(), pcpu.data(), pmem.data(),
                   px.data(), movable.data(), drainPolicy, M, summary, shc.data(), shm.data(),
                   shx.data(), shn.data(), shp.data(), shu.data(), she.data());
    if (rc) return fail(ctx, rc);
    if (summary[2] < 0) {
      std::printf("Drained %" PRId64 " nodes : %" PRId64 " pods evicted, shapes exceed %" PRId64
                  ": none placed\n", summary[0], summary[1], M);
    } else {
      std::printf("Drained %" PRId64 " nodes : %" PRId64 " pods evicted, %" PRId64 " placed, %" PRId64
                  " not placed (%" PRId64 " shapes)\n", summary[0], summary[1], summary[3],
                  summary[1] - summary[3], summary[2]);
      for (int64_t j = 0; j < summary[2]; ++j)
        if (she[(size_t)j])
          std::printf("Drain shape %" PRIu64 "m %" PRId64 " : %" PRId64 " pods not placed, a zero request "
                      "(panic: runtime error: integer divide by zero)\n", shc[(size_t)j], shm[(size_t)j],
                      shn[(size_t)j]);
    }
    suc = euc;
    sum_ = eum;
  }

  // -consolidate: for each candidate node on its own, its pods (requests and `daemon` pods as
  // -drain's) placed on the other nodes as they stand, by kcc_consolidate.  The state is only
  // read: the fits below are what they are without the flag.
  if (consOn) {
    std::vector<uint64_t> cuc(euc);
    std::vector<int64_t> cum(eum);
    if (!useExt) {  // the per-node request sums (CC:290-293)
      cuc.assign((size_t)n, 0);
      cum.assign((size_t)n, 0);
      rc = kcc_reduce_requests(ctx, n, nc, in.node_ptr.data(), in.cpu_req.data(), in.mem_req.data(),
                               nullptr, nullptr, cuc.data(), cum.data(), nullptr, nullptr);
      if (rc) return fail(ctx, rc);
    }
    // an unhealthy node is never a candidate: its row is a zero row and lists no pods
    std::vector<uint8_t> pick((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i) {
      if (rows[(size_t)i].name.empty()) continue;
      if (consKind == "all") {
        pick[(size_t)i] = 1;
      } else if (consKind == "below") {  // the scale-down threshold: used * 100 < pct * alloc, both
        const unsigned __int128 uc = cuc[(size_t)i], ac = in.alloc_cpu[(size_t)i];
        const __int128 um = cum[(size_t)i], am = in.alloc_mem[(size_t)i];
        pick[(size_t)i] = uc * 100 < ac * (unsigned __int128)consPct && um * 100 < am * (__int128)consPct;
      }
    }
    for (const std::string& want : consNames) {
      bool found = false;
      for (int64_t i = 0; i < n; ++i) {
        if (cl.nodes[(size_t)i].name != want) continue;
        if (!rows[(size_t)i].name.empty()) pick[(size_t)i] = 1;
        found = true;
      }
      if (!found) {
        std::fprintf(stderr, "-consolidate: no node with name %s in %s\n", want.c_str(), path.c_str());
        kcc_destroy(ctx);
        return 1;
      }
    }
    std::vector<int64_t> cand;
    for (int64_t i = 0; i < n; ++i)
      if (pick[(size_t)i]) cand.push_back(i);
    const size_t P = in.pod_daemon.size(), Cn = cand.size();
    std::vector<uint64_t> pcpu;
    std::vector<int64_t> pmem, px;
    std::vector<uint8_t> movable;
    podRequests(pcpu, pmem, px, movable);
    std::vector<int64_t> cev(Cn), cpl(Cn), cze(Cn);
    std::vector<int32_t> cer(Cn);
    rc = kcc_consolidate(ctx, n, in.alloc_cpu.data(), in.alloc_mem.data(), in.alloc_pods.data(),
                         ext.R(), ext.alloc_x.data(), in.pod_count.data(), cuc.data(), cum.data(),
                         ext.used_x.data(), nullptr, (int64_t)P, in.lv_node_pod_ptr.data(),
                         pcpu.data(), pmem.data(), px.data(), movable.data(), (int64_t)Cn,
                         cand.data(), cev.data(), cpl.data(), cze.data(), cer.data(), nullptr);
    if (rc) return fail(ctx, rc);
    int64_t strict = 0, lenient = 0;
    for (size_t j = 0; j < Cn; ++j) {
      const char* name = cl.nodes[(size_t)cand[j]].name.c_str();
      if (cer[j] == KCC_CAND_TOOMANY) {
        std::printf("Node %s : %" PRId64 " pods evicted, more than %d: not evaluated\n", name, cev[j],
                    KCC_CONS_MAX_PODS);
        continue;
      }
      std::printf("Node %s : %" PRId64 " pods evicted, %" PRId64 " placed, %" PRId64 " not placed, %" PRId64
                  " without requests\n", name, cev[j], cpl[j], cev[j] - cpl[j] - cze[j], cze[j]);
      strict += cer[j] == KCC_CAND_OK && cpl[j] == cev[j];
      lenient += cer[j] == KCC_CAND_OK && cpl[j] + cze[j] == cev[j];
    }
    std::printf("Removable one at a time : %" PRId64 " of %zu nodes (%" PRId64
                " counting pods without requests as placed)\n", strict, Cn, lenient);
  }

  if (verbose) {  // CC:107-117, 137 — per-node sums and fit, one row at a time
    std::vector<uint64_t> uc(n), lc(n);
    std::vector<int64_t> um(n), lm(n);
    rc = kcc_reduce_requests(ctx, n, nc, in.node_ptr.data(), in.cpu_req.data(), in.mem_req.data(),
                             in.cpu_lim.data(), in.mem_lim.data(), uc.data(), um.data(), lc.data(),
                             lm.data());
    if (rc) return fail(ctx, rc);
    if (schedReq) {
      uc = suc;
      um = sum_;
    }
    // every row's "Max replicas" (CC:137) for the first spec in one device call
    std::vector<int64_t> qs(n);
    std::vector<int32_t> es(n);
    if (useExt) {  // every row its own group: cell i is row i's q for the first spec
      std::vector<int32_t> each((size_t)n);
      for (int64_t i = 0; i < n; ++i) each[(size_t)i] = (int32_t)i;
      std::vector<int64_t> x0((size_t)ext.R());
      for (int64_t r = 0; r < ext.R(); ++r) x0[(size_t)r] = ext.spec_x[(size_t)(r * S)];
      if (n > 0)
        rc = kcc_fit_ext(ctx, n, in.alloc_cpu.data(), in.alloc_mem.data(), in.alloc_pods.data(),
                         in.pod_count.data(), uc.data(), um.data(), ext.R(), ext.alloc_x.data(),
                         ext.used_x.data(), each.data(), n, 1, &specs[0].cpu, &specs[0].mem,
                         x0.data(), qs.data(), es.data());
    } else {
      rc = kcc_fit_rows(ctx, n, in.alloc_cpu.data(), in.alloc_mem.data(), in.alloc_pods.data(),
                        in.pod_count.data(), uc.data(), um.data(), specs[0].cpu, specs[0].mem,
                        qs.data(), es.data());
    }
    if (rc) return fail(ctx, rc);
    for (int64_t i = 0; i < n; ++i) {
      const int64_t q = qs[i];
      const int32_t e = es[i];
      std::printf("\n{%s %" PRIu64 " %" PRId64 " %" PRId64 "} - Current non-terminated pods : %" PRId64,
                  rows[i].name.c_str(), rows[i].allocatableCPU, rows[i].allocatableMemory,
                  rows[i].allocatablePods, in.pod_count[i]);
      std::printf("\nSum of CPU Limits, Requests and Memory Limits, Requests for all pods : %" PRIu64
                  " %" PRIu64 " %" PRId64 " %" PRId64, lc[i], uc[i], lm[i], um[i]);
      std::printf("\nTotal allocatbale CPU and Memory : %" PRIu64 ", %" PRId64, rows[i].allocatableCPU,
                  rows[i].allocatableMemory);
      const double ac = (double)rows[i].allocatableCPU, am = (double)rows[i].allocatableMemory;
      std::printf("\nCPU Limits, Requests and Memory Limits, Requests used percentage till now : "
                  "%s %s %s %s", goF2((double)lc[i] * 100 / ac).c_str(),
                  goF2((double)uc[i] * 100 / ac).c_str(), goF2((double)lm[i] * 100 / am).c_str(),
                  goF2((double)um[i] * 100 / am).c_str());
      if (e) {
        std::fprintf(stderr, "panic: runtime error: integer divide by zero\n");
        kcc_destroy(ctx);
        return 2;
      }
      std::printf("\nMax replicas : %" PRId64 "\n", q);
    }
  }

  std::vector<uint64_t> sc(specs.size());
  std::vector<int64_t> sm(specs.size()), totals(specs.size());
  std::vector<int32_t> serr(specs.size());
  for (size_t s = 0; s < specs.size(); ++s) {
    sc[s] = specs[s].cpu;
    sm[s] = specs[s].mem;
  }
  if (useExt)
    rc = kcc_fit_ext(ctx, n, in.alloc_cpu.data(), in.alloc_mem.data(), in.alloc_pods.data(),
                     in.pod_count.data(), euc.data(), eum.data(), ext.R(), ext.alloc_x.data(),
                     ext.used_x.data(), nullptr, 1, S, sc.data(), sm.data(), ext.spec_x.data(),
                     totals.data(), serr.data());
  else if (explicitSums)
    rc = kcc_fit(ctx, n, in.alloc_cpu.data(), in.alloc_mem.data(), in.alloc_pods.data(),
                 in.pod_count.data(), suc.data(), sum_.data(), (int64_t)specs.size(), sc.data(),
                 sm.data(), totals.data(), serr.data());
  else
    rc = kcc_capacity(ctx, n, nc, in.node_ptr.data(), in.cpu_req.data(), in.mem_req.data(),
                      in.alloc_cpu.data(), in.alloc_mem.data(), in.alloc_pods.data(),
                      in.pod_count.data(), (int64_t)specs.size(), sc.data(), sm.data(),
                      totals.data(), serr.data());
  if (rc) return fail(ctx, rc);

  // -maxPerNode / -spreadBy zone: the totals again under the spread constraints.  Row i is in
  // the zone of node i (zones in first-appearance order; without -spreadBy one group);
  // ztot / zerr [zone][spec] are the zones' capacities under the per-node cap.
  std::vector<std::string> zones;
  std::vector<int64_t> ztot, zrows;
  std::vector<int32_t> zerr;
  const std::vector<int64_t> caps(specs.size(), maxPerNode);
  if (spread && n > 0) {
    std::vector<int32_t> group;
    if (byZone) {
      std::map<std::string, int32_t> id;
      group.resize((size_t)n);
      for (int64_t i = 0; i < n; ++i) {
        const std::string& name = cl.nodes[(size_t)i].zone;
        auto it = id.find(name);
        if (it == id.end()) {
          it = id.emplace(name, (int32_t)zones.size()).first;
          zones.push_back(name);
        }
        group[(size_t)i] = it->second;
      }
    }
    const int64_t Z = byZone ? (int64_t)zones.size() : 1;
    std::vector<uint64_t> uc(useExt ? euc : suc);
    std::vector<int64_t> um(useExt ? eum : sum_);
    if (!useExt && !explicitSums) {  // the per-node request sums (CC:290-293)
      uc.resize((size_t)n);
      um.resize((size_t)n);
      rc = kcc_reduce_requests(ctx, n, nc, in.node_ptr.data(), in.cpu_req.data(),
                               in.mem_req.data(), nullptr, nullptr, uc.data(), um.data(), nullptr,
                               nullptr);
      if (rc) return fail(ctx, rc);
    }
    ztot.resize((size_t)(Z * S));
    zerr.resize((size_t)(Z * S));
    zrows.resize((size_t)Z);
    rc = kcc_fit_capped(ctx, n, in.alloc_cpu.data(), in.alloc_mem.data(), in.alloc_pods.data(),
                        in.pod_count.data(), uc.data(), um.data(), ext.R(), ext.alloc_x.data(),
                        ext.used_x.data(), byZone ? group.data() : nullptr, Z, S, sc.data(),
                        sm.data(), ext.spec_x.data(), ztot.data(), zerr.data(), caps.data(),
                        nullptr, zrows.data());  // (without extended resources ext is empty: R 0)
    if (rc) return fail(ctx, rc);
    const std::vector<int64_t> skew(specs.size(), byZone ? maxSkew : 0);
    rc = kcc_spread_fold(ctx, Z, S, ztot.data(), zerr.data(), zrows.data(), nullptr, Z, nullptr,
                         skew.data(), totals.data(), serr.data());
    if (rc) return fail(ctx, rc);
  }
  // "Zone <name> : <used> of <cap>": used = min(cap, the smallest zone's cap + maxSkew)
  auto printZones = [&](size_t s) {
    if (zones.empty()) return;
    int64_t m = INT64_MAX;
    for (size_t z = 0; z < zones.size(); ++z)
      if (ztot[z * specs.size() + s] < m) m = ztot[z * specs.size() + s];
    const int64_t lim = (m > 0 && maxSkew > INT64_MAX - m) ? INT64_MAX : m + maxSkew;
    for (size_t z = 0; z < zones.size(); ++z) {
      const int64_t cap = ztot[z * specs.size() + s];
      if (zerr[z * specs.size() + s])
        std::printf("Zone %s : panic: runtime error: integer divide by zero\n", zones[z].c_str());
      else if (serr[s])
        std::printf("Zone %s : - of %" PRId64 "\n", zones[z].c_str(), cap);
      else
        std::printf("Zone %s : %" PRId64 " of %" PRId64 "\n", zones[z].c_str(), cap <= lim ? cap : lim,
                    cap);
    }
  };

  // -byPool: row i is in the pool of node i (an unhealthy node's zero row stays in its
  // node's pool); pools in first-appearance order; ptot / perr [pool][spec]
  std::vector<std::string> pools;
  std::vector<int64_t> ptot;
  std::vector<int32_t> perr;
  std::vector<int32_t> poolGroup;  // (-priority reads the pools' ids again)
  if (byPool && n > 0) {
    std::map<std::string, int32_t> id;
    std::vector<int32_t>& group = poolGroup;
    group.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
      const std::string& name = cl.nodes[(size_t)i].pool;
      auto it = id.find(name);
      if (it == id.end()) {
        it = id.emplace(name, (int32_t)pools.size()).first;
        pools.push_back(name);
      }
      group[(size_t)i] = it->second;
    }
    std::vector<uint64_t> uc(suc);
    std::vector<int64_t> um(sum_);
    if (!explicitSums) {  // the per-node request sums (CC:290-293) the grouped fit takes
      uc.resize((size_t)n);
      um.resize((size_t)n);
      rc = kcc_reduce_requests(ctx, n, nc, in.node_ptr.data(), in.cpu_req.data(),
                               in.mem_req.data(), nullptr, nullptr, uc.data(), um.data(), nullptr,
                               nullptr);
      if (rc) return fail(ctx, rc);
    }
    ptot.resize(pools.size() * specs.size());
    perr.resize(pools.size() * specs.size());
    // one call: the pools under the per-node cap if there is one, with the extended
    // resources if there are any (without them ext is empty: R 0) — else the grouped fit
    rc = kcc_fit_capped(ctx, n, in.alloc_cpu.data(), in.alloc_mem.data(), in.alloc_pods.data(),
                        in.pod_count.data(), uc.data(), um.data(), ext.R(), ext.alloc_x.data(),
                        ext.used_x.data(), group.data(), (int64_t)pools.size(), S, sc.data(),
                        sm.data(), ext.spec_x.data(), ptot.data(), perr.data(),
                        maxPerNode > 0 ? caps.data() : nullptr, nullptr, nullptr);
    if (rc) return fail(ctx, rc);
  }
  auto printPools = [&](size_t s) {
    for (size_t g = 0; g < pools.size(); ++g) {
      if (perr[g * specs.size() + s])
        std::printf("Pool %s : panic: runtime error: integer divide by zero\n", pools[g].c_str());
      else
        std::printf("Pool %s : %" PRId64 "\n", pools[g].c_str(), ptot[g * specs.size() + s]);
    }
  };
  // -explain: the reasons and the leftovers of every spec's total in one ungrouped call, on
  // the sums and the cap that total came from; wrows / wpods [slot][spec], left [resource][spec]
  std::vector<int64_t> wrows, wpods, left;
  if (explain && S > 0) {
    std::vector<uint64_t> uc(useExt ? euc : suc);
    std::vector<int64_t> um(useExt ? eum : sum_);
    if (!useExt && !explicitSums) {  // the per-node request sums (CC:290-293)
      uc.resize((size_t)n);
      um.resize((size_t)n);
      rc = kcc_reduce_requests(ctx, n, nc, in.node_ptr.data(), in.cpu_req.data(),
                               in.mem_req.data(), nullptr, nullptr, uc.data(), um.data(), nullptr,
                               nullptr);
      if (rc) return fail(ctx, rc);
    }
    std::vector<int64_t> et((size_t)S);
    std::vector<int32_t> ee((size_t)S);
    wrows.resize((size_t)(KCC_WHY_SLOTS * S));
    wpods.resize((size_t)(KCC_WHY_SLOTS * S));
    left.resize((size_t)((2 + ext.R()) * S));
    rc = kcc_fit_explain(ctx, n, in.alloc_cpu.data(), in.alloc_mem.data(), in.alloc_pods.data(),
                         in.pod_count.data(), uc.data(), um.data(), ext.R(), ext.alloc_x.data(),
                         ext.used_x.data(), nullptr, 1, S, sc.data(), sm.data(), ext.spec_x.data(),
                         maxPerNode > 0 ? caps.data() : nullptr, et.data(), ee.data(),
                         wrows.data(), wpods.data(), left.data());
    if (rc) return fail(ctx, rc);
  }
  // -priority: two levels of node state in one pass over the containers (the extended
  // resources' columns two a call, in the cpu_req / mem_req places), then every spec on plane 1;
  // ltot / lerr [spec], lptot / lperr [pool][spec], evicted = the pods below the priority
  std::vector<int64_t> ltot((size_t)S, 0), lptot(pools.size() * (size_t)S, 0);
  std::vector<int32_t> lerr((size_t)S, 0), lperr(pools.size() * (size_t)S, 0);
  int64_t evicted = 0;
  if (prioOn && n > 0) {
    const int64_t P = (int64_t)in.pod_priority.size(), R = ext.R();
    std::vector<uint8_t> level((size_t)P);
    for (int64_t p = 0; p < P; ++p) level[(size_t)p] = in.pod_priority[(size_t)p] >= prio ? 1 : 0;
    std::vector<uint64_t> luc((size_t)(2 * n));
    std::vector<int64_t> lum((size_t)(2 * n)), lpc((size_t)(2 * n)), lux((size_t)(2 * R * n), 0);
    rc = kcc_reduce_requests_levels(ctx, n, P, nc, in.lv_node_pod_ptr.data(), in.lv_pod_ptr.data(),
                                    in.cpu_req.data(), in.mem_req.data(), level.data(), 2,
                                    luc.data(), lum.data(), lpc.data());
    if (rc) return fail(ctx, rc);
    for (int64_t i = 0; i < n; ++i) evicted += lpc[(size_t)i] - lpc[(size_t)(n + i)];
    for (int64_t r0 = 0; r0 < R; r0 += 2) {
      std::vector<uint64_t> c0((size_t)nc, 0), o0((size_t)(2 * n));
      std::vector<int64_t> c1((size_t)nc, 0), o1((size_t)(2 * n)), cnt((size_t)(2 * n));
      for (int64_t k = 0; k < nc; ++k) {
        const auto it = ext.creq.find(in.app[(size_t)k]);
        if (it == ext.creq.end()) continue;
        c0[(size_t)k] = (uint64_t)it->second[(size_t)r0];
        if (r0 + 1 < R) c1[(size_t)k] = it->second[(size_t)r0 + 1];
      }
      rc = kcc_reduce_requests_levels(ctx, n, P, nc, in.lv_node_pod_ptr.data(), in.lv_pod_ptr.data(),
                                      c0.data(), c1.data(), level.data(), 2, o0.data(), o1.data(),
                                      cnt.data());
      if (rc) return fail(ctx, rc);
      for (int64_t l = 0; l < 2; ++l)
        for (int64_t i = 0; i < n; ++i) {
          lux[(size_t)((l * R + r0) * n + i)] = (int64_t)o0[(size_t)(l * n + i)];
          if (r0 + 1 < R) lux[(size_t)((l * R + r0 + 1) * n + i)] = o1[(size_t)(l * n + i)];
        }
    }
    const int64_t level_ptr[3] = {0, 0, S};  // every spec at level 1
    const int64_t* cap = maxPerNode > 0 ? caps.data() : nullptr;
    rc = kcc_fit_levels(ctx, n, in.alloc_cpu.data(), in.alloc_mem.data(), in.alloc_pods.data(), 2,
                        lpc.data(), luc.data(), lum.data(), R, ext.alloc_x.data(), lux.data(), nullptr,
                        1, S, sc.data(), sm.data(), ext.spec_x.data(), cap, level_ptr, ltot.data(),
                        lerr.data());
    if (rc) return fail(ctx, rc);
    if (!pools.empty()) {
      rc = kcc_fit_levels(ctx, n, in.alloc_cpu.data(), in.alloc_mem.data(), in.alloc_pods.data(), 2,
                          lpc.data(), luc.data(), lum.data(), R, ext.alloc_x.data(), lux.data(),
                          poolGroup.data(), (int64_t)pools.size(), S, sc.data(), sm.data(),
                          ext.spec_x.data(), cap, level_ptr, lptot.data(), lperr.data());
      if (rc) return fail(ctx, rc);
    }
  }
  auto printPreempt = [&](size_t s) {
    if (!prioOn) return;
    if (lerr[s])
      std::printf("With preemption of pods below priority %" PRId64 " : panic: runtime error: integer divide by zero\n", prio);
    else
      std::printf("With preemption of pods below priority %" PRId64 " : %" PRId64 ", at most %" PRId64
                  " pods evicted\n", prio, ltot[s], evicted);
  };
  auto printPreemptPools = [&](size_t s) {
    if (!prioOn) return;
    for (size_t g = 0; g < pools.size(); ++g) {
      if (lperr[g * specs.size() + s])
        std::printf("Pool %s with preemption : panic: runtime error: integer divide by zero\n", pools[g].c_str());
      else
        std::printf("Pool %s with preemption : %" PRId64 "\n", pools[g].c_str(), lptot[g * specs.size() + s]);
    }
  };
  auto printExplain = [&](size_t s) {
    if (!explain || serr[s]) return;
    for (int b = 0; b < KCC_WHY_SLOTS; ++b) {
      const int64_t rws = wrows[(size_t)b * specs.size() + s];
      if (rws == 0) continue;
      const char* name = b == KCC_WHY_CPU    ? "cpu"
                         : b == KCC_WHY_MEM  ? "memory"
                         : b == KCC_WHY_PODS ? "pods"
                         : b == KCC_WHY_CAP  ? "perNode"
                                             : ext.names[(size_t)(b - KCC_WHY_EXT0)].c_str();
      std::printf("Limited by %s : %" PRId64 " nodes, %" PRId64 " replicas\n", name, rws,
                  wpods[(size_t)b * specs.size() + s]);
    }
    std::printf("Left over cpu : %" PRId64 "m\n", left[s]);
    std::printf("Left over memory : %" PRId64 "\n", left[specs.size() + s]);
    for (size_t r = 0; r < (size_t)ext.R(); ++r)
      std::printf("Left over %s : %" PRId64 "\n", ext.names[r].c_str(),
                  left[(2 + r) * specs.size() + s]);
  };
  kcc_destroy(ctx);

  if (f.v["specs"].empty()) {  // CC:142-149, verbatim text
    if (serr[0]) {
      std::fprintf(stderr, "panic: runtime error: integer divide by zero\n");
      return 2;
    }
    std::printf("%s\n", kRule);
    std::printf("\n\t Total possible replicas for the pod with required input specs : %" PRId64,
                totals[0]);
    if (totals[0] >= specs[0].replicas)
      std::printf("\n\t So you can go ahead with deployment of %" PRId64
                  " pod replicas in the Kubernetes cluster!!\n\n", specs[0].replicas);
    else
      std::printf("\n\t Unfortunately Kubernetes cluster can't scehdule %" PRId64
                  " replicas. Please try again by reducing the number of replicas or/and cpu/memory "
                  "resource requests. Exiting!!\n\n", specs[0].replicas);
    std::printf("%s\n", kRule);
    printPreempt(0);
    printExplain(0);
    printZones(0);
    printPools(0);
    printPreemptPools(0);
    return 0;
  }
  // batch: one line per spec
  for (size_t s = 0; s < specs.size(); ++s) {
    if (serr[s])
      std::printf("%s %s %s panic: integer divide by zero\n", specs[s].cpuStr.c_str(),
                  specs[s].memStr.c_str(), specs[s].repStr.c_str());
    else
      std::printf("%s %s %s total=%" PRId64 " %s\n", specs[s].cpuStr.c_str(), specs[s].memStr.c_str(),
                  specs[s].repStr.c_str(), totals[s], totals[s] >= specs[s].replicas ? "yes" : "no");
    printPreempt(s);  // (-priority: this spec's total with preemption under its line)
    printExplain(s);  // (-explain: this spec's reasons and leftovers under its line)
    printZones(s);  // (-spreadBy zone: this spec's zones under its line)
    printPools(s);  // (-byPool: this spec's pools under its line)
    printPreemptPools(s);
  }
  return 0;
}
