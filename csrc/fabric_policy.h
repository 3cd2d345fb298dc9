// The two decisions of the queue fabric as pure functions of numbers: which consumer gets a produced
// frame (route), and how a consumer shares its free slots among its producers (grants).  No HIP, no
// links, no atomics, no locks: QueueFabric reads the mailboxes and the pool, calls these, and applies
// the answer (fabric.cpp: route_produced, grant_free_slots); tests/test_fabric_policy.py calls them
// directly.  The constants (QueueFabric::kLocalSlack, kFeedLocalReady, kMinGrants) are passed in.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace pr {
namespace fabric_policy {

// ---------------------------------------------------------------------------------------
// Route

struct RouteCand {          // one outgoing link that can take frames now
  int64_t avail = 0;        // grants held
  bool keeper = false;      // the consumer end is a queue keeper
  // balanced only: a consumer-ONLY member (no producer of its own feeds it) that published its
  // demand and has nothing to read (the caller reads the mailbox)
  bool may_starve = false;
};

struct Routed {
  std::vector<int> local;                 // offers for this process's own consumer
  std::vector<std::vector<int>> assign;   // offers per candidate
  std::vector<int> left;                  // offers nobody has credit for (they stay in the FIFO)
  int rr = 0;                             // spread: where the next pass starts its round
  int64_t local_credit = 0;               // what the local routes left of it
};

// Produced frames (FIFO) to this process's own consumer or to granted remote slots.  `local_credit`
// arrives after the relay / remote_only / spread adjustments.  Keeper links are the last resort: a
// frame goes there only when no real consumer (and not this process's own) has credit for it.
inline Routed route(int policy, const std::vector<int>& offers, const std::vector<RouteCand>& cands,
                    int64_t local_credit, int64_t n_ready, int rr, int local_slack, int feed_local_ready) {
  Routed r;
  r.assign.resize(cands.size());
  r.rr = rr;
  std::vector<int64_t> avail(cands.size());
  for (size_t i = 0; i < cands.size(); ++i) avail[i] = cands[i].avail;
  const int K = (int)cands.size() + 1;   // position K-1 = this process's own consumer
  // balanced: a remote consumer-ONLY member (no producer of its own feeds it) with NOTHING to
  // read (its published ready count is 0) and credit here is starving -- competing consumers pull
  // from one queue in the reference (shared_queue.py:19-24), so it is fed first while our own
  // consumer has frames ready (a consumer-only rank next to a fast co-located consumer would
  // otherwise never see a frame; BASELINE config 3).  Consumers that produce for themselves are
  // left to their own producer, so the weak-scaling case stays local.  Each offer goes to the
  // starving member given the fewest in this pass (several starving members share); a copy to it
  // still in flight does not stop the feed (waiting for it idled the member one notice -> copy ->
  // notice round trip per refill), its grants -- its read-ahead bound -- do.
  std::vector<int> starving;
  if (policy == 0 && (local_credit <= 0 || n_ready >= feed_local_ready))
    for (size_t i = 0; i < cands.size(); ++i)
      if (!cands[i].keeper && avail[i] > 0 && cands[i].may_starve) starving.push_back((int)i);
  size_t o = 0;
  for (; o < offers.size(); ++o) {
    const int s = offers[o];
    int pick = -2;   // -2 none, -1 local, >= 0 remote
    int sp = -1;
    for (int i : starving)
      if (avail[i] > 0 && (sp < 0 || r.assign[i].size() < r.assign[sp].size())) sp = i;
    if (sp >= 0) {
      r.assign[sp].push_back(s);
      --avail[sp];
      continue;
    }
    if (policy == 2) {
      for (int t = 0; t < K && pick == -2; ++t) {
        const int p = (r.rr + t) % K;
        if (p == K - 1) {
          if (local_credit > 0) pick = -1;
        } else if (avail[p] > 0 && !cands[p].keeper) {
          pick = p;
        }
        if (pick != -2) r.rr = (p + 1) % K;
      }
    } else {
      int best = -1;
      for (size_t i = 0; i < cands.size(); ++i)
        if (avail[i] > 0 && !cands[i].keeper && (best < 0 || avail[i] > avail[best])) best = (int)i;
      const int64_t best_n = best >= 0 ? avail[best] : 0;
      if (local_credit > 0 && (policy == 1 || local_credit + local_slack >= best_n)) pick = -1;
      else if (best >= 0) pick = best;
    }
    if (pick == -2)   // nobody else: a keeper with credit
      for (size_t i = 0; i < cands.size(); ++i)
        if (avail[i] > 0 && cands[i].keeper) {
          pick = (int)i;
          break;
        }
    if (pick == -2) break;
    if (pick == -1) {
      r.local.push_back(s);
      --local_credit;
    } else {
      r.assign[pick].push_back(s);
      --avail[pick];
    }
  }
  r.left.assign(offers.begin() + (std::ptrdiff_t)o, offers.end());
  r.local_credit = local_credit;
  return r;
}

// ---------------------------------------------------------------------------------------
// Grants

// grants a consumer keeps at each of its `n` live producers, whatever their backlog
inline int grant_floor(int cb, int n, int min_grants) { return std::max(min_grants, std::min(64, cb / (2 * n))); }

// spread: the own producer must not take the consumer credit that the remote producers' grants
// need.  A local route needs only credit, a grant needs a FREE slot whose release event has
// completed -- so without a reservation the local route wins every race and all frames stay local.
// Each live remote producer's grant floor stays reserved: what is missing of it is the reserve.
inline int64_t spread_reserve(int cb, const std::vector<int64_t>& outstanding, int min_grants) {
  if (outstanding.empty()) return 0;
  const int64_t floor_g = grant_floor(cb, (int)outstanding.size(), min_grants);
  int64_t reserve = 0;
  for (int64_t o : outstanding) reserve += std::max<int64_t>(0, floor_g - o);
  return reserve;
}

struct GrantWants {
  std::vector<int64_t> want;   // per producer
  int64_t total = 0;           // slots to ask the pool for
};

// What each live producer should still be granted (its floor plus its backlog, less what it holds
// unanswered), and their sum capped by the read-ahead allowance: `cb`, or `prefetch - held` when a
// prefetch is set (held = frames noticed but not taken + grants outstanding).
inline GrantWants grant_wants(int cb, const std::vector<int64_t>& backlog, const std::vector<int64_t>& outstanding,
                              int prefetch, int64_t held, int min_grants) {
  GrantWants g;
  const size_t n = backlog.size();
  g.want.resize(n);
  if (n == 0) return g;
  const int64_t allowance = prefetch > 0 ? std::max<int64_t>(0, (int64_t)prefetch - held) : cb;
  const int floor_g = grant_floor(cb, (int)n, min_grants);
  for (size_t i = 0; i < n; ++i) {
    g.want[i] = std::max<int64_t>(0, std::min<int64_t>(cb, floor_g + std::max<int64_t>(0, backlog[i])) - outstanding[i]);
    g.total += g.want[i];
  }
  g.total = std::min(g.total, allowance);
  return g;
}

// The producer that gets each of `k` granted slots, in order: round-robin over the producers that
// still want one, so concurrent demand shares the free slots.  Shorter than k when the wants run out.
inline std::vector<int> grant_deal(std::vector<int64_t> want, size_t k) {
  std::vector<int> to;
  to.reserve(k);
  while (to.size() < k) {
    bool any = false;
    for (size_t i = 0; i < want.size() && to.size() < k; ++i) {
      if (want[i] <= 0) continue;
      to.push_back((int)i);
      --want[i];
      any = true;
    }
    if (!any) break;
  }
  return to;
}

}  // namespace fabric_policy
}  // namespace pr
