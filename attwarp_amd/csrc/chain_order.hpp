// Block order of the one-launch steps of the main_batched chain (chain_step.hip: equally shaped batches;
// chain_ragged.hip: differently sized images): the grid holds the blocks of five stages -- F, V, P, L, R -- of five
// different batches.  F and V blocks first (the longest dependent chains start at once), then all of P (its blocks walk
// every row of a column strip and are the longest-lived of the launch: dispatched late they would be its tail), then L
// and R interleaved in proportion to their counts, then what the whole periods of the interleave left of L and of R.
// Everything is laid out in units of 8 consecutive blocks ("octets") so that block % 8 keeps naming the XCD for the
// resample's XCD-aware order.
#pragma once
#include "common.hpp"

#include <cstring>

namespace attwarp {

constexpr int CHAIN_Q = 32;                 // octets per period of the L / R interleave

struct ChainOrder {
  int nF, nV, nP, nL, nR;                   // blocks of F, V, P, L, R
  int nF8, nV8, nP8;                        // octets of the F, V and P ranges
  // interleave: `periods` periods of CHAIN_Q octets, each holding q[t] octets of kind t (0 = L, 1 = R) at the positions
  // type[] says (rank[] = how many octets of the same kind precede inside the period); then the left8[0] octets of L and
  // the left8[1] octets of R that the whole periods left, one range after the other
  int periods, q[2], left8[2];
  unsigned char type[CHAIN_Q], rank[CHAIN_Q];
};

enum { CHAIN_F = 0, CHAIN_V = 1, CHAIN_P = 2, CHAIN_L = 3, CHAIN_R = 4, CHAIN_PAD = -1 };

#ifdef __HIPCC__
// block `blk` of the grid -> its kind and its index j inside that kind's range (CHAIN_PAD: a padding block)
__device__ __forceinline__ int chain_order_decode(const ChainOrder& a, int blk, int& j) {
  const int l8 = blk & 7;
  int oct = blk >> 3;
  if (oct < a.nF8) { j = blk; return blk < a.nF ? CHAIN_F : CHAIN_PAD; }
  oct -= a.nF8;
  if (oct < a.nV8) { j = oct * 8 + l8; return j < a.nV ? CHAIN_V : CHAIN_PAD; }
  oct -= a.nV8;
  if (oct < a.nP8) { j = oct * 8 + l8; return j < a.nP ? CHAIN_P : CHAIN_PAD; }
  oct -= a.nP8;
  int t, idx8;
  if (oct < a.periods * CHAIN_Q) {
    const int per = oct / CHAIN_Q, pos = oct - per * CHAIN_Q;
    t = a.type[pos];
    idx8 = per * a.q[t] + a.rank[pos];
  } else {                                  // the leftovers start where the whole periods stopped in each kind
    int r = oct - a.periods * CHAIN_Q;
    t = r < a.left8[0] ? 0 : 1;
    if (t) r -= a.left8[0];
    idx8 = a.periods * a.q[t] + r;
  }
  j = idx8 * 8 + l8;
  if (t == 0) return j < a.nL ? CHAIN_L : CHAIN_PAD;
  return j < a.nR ? CHAIN_R : CHAIN_PAD;
}
#endif

// Fills the octet counts and the L / R interleave from nF .. nR.  The interleave: q[] by largest-remainder rounding of
// each kind's share of a period, then an even spread (position i goes to the kind that is furthest behind its share),
// as many whole periods as both kinds fill.
inline void build_interleave(ChainOrder& a) {
  a.nF8 = (a.nF + 7) / 8;
  a.nV8 = (a.nV + 7) / 8;
  a.nP8 = (a.nP + 7) / 8;
  const int n8[2] = {(a.nL + 7) / 8, (a.nR + 7) / 8};
  a.periods = 0;
  a.q[0] = a.q[1] = 0;
  memset(a.type, 0, sizeof(a.type));
  memset(a.rank, 0, sizeof(a.rank));
  const long long tot = (long long)n8[0] + n8[1];
  if (tot > 0) {
    int q[2], used = 0;
    double frac[2];
    for (int t = 0; t < 2; ++t) {
      const double share = (double)CHAIN_Q * n8[t] / (double)tot;
      q[t] = (int)share;
      if (n8[t] > 0 && q[t] == 0) q[t] = 1;
      frac[t] = share - (int)share;
      used += q[t];
    }
    while (used < CHAIN_Q) {
      const int best = frac[1] > frac[0] ? 1 : 0;
      ++q[best]; frac[best] = -1.0; ++used;
    }
    while (used > CHAIN_Q) {
      const int big = q[1] > q[0] ? 1 : 0;
      --q[big]; --used;
    }
    int periods = 0x7fffffff;
    for (int t = 0; t < 2; ++t) if (q[t] > 0) periods = std::min(periods, n8[t] / q[t]);
    a.periods = periods == 0x7fffffff ? 0 : periods;
    int placed[2] = {0, 0};
    for (int i = 0; i < CHAIN_Q; ++i) {
      int best = -1;
      double lag = -1e30;
      for (int t = 0; t < 2; ++t) {
        if (placed[t] >= q[t]) continue;
        const double l = (double)(i + 1) * q[t] / CHAIN_Q - placed[t];
        if (l > lag) { lag = l; best = t; }
      }
      a.type[i] = (unsigned char)best;
      a.rank[i] = (unsigned char)placed[best];
      ++placed[best];
    }
    a.q[0] = q[0]; a.q[1] = q[1];
  }
  for (int t = 0; t < 2; ++t) a.left8[t] = n8[t] - a.periods * a.q[t];
}

// octets of the whole grid once build_interleave has run
inline long long chain_order_octets(const ChainOrder& a) {
  return (long long)a.nF8 + a.nV8 + a.nP8 + (long long)a.periods * CHAIN_Q + a.left8[0] + a.left8[1];
}

}  // namespace attwarp
