// peaq_group_sched.h -- the schedule of the front end's critical-band sums (peaq_frontend.hip, fftearmodel.c:604-620):
// which LDS read of which lane fetches which bin.  Plain constexpr functions, usable from host code: the kernel takes
// its slot counts and predicates from here, peaq_tables.cpp holds the band tables against the counts when a context is
// created, and tools/group_sched_check.cpp runs the same schedule on an array against the plain loop.
//
// The setting: lane L < (NB + 1) / 2 sums band L ("narrow") and band NB - 1 - L ("wide").  A band is
//   wlo Pw[lo] + whi Pw[hi] + Pw[lo + 1] + ... + Pw[hi - 1]
// in that order.  The interior bins are contiguous doubles in LDS, so they are fetched two per read ("pair slot" j
// reads the bins lo + 1 + 2 j and lo + 2 + 2 j) with a FIXED number of slots per band -- no loop whose trip count is the
// longest band of the wave -- and one single read for the odd bin hi - 1 that is left over.  A slot beyond the band's end
// reads a pair of zero words: the caller keeps group_zero_words of them from `zero` on, so that ONE base serves every
// idle slot (slot j's constant 2 j sits in the read's offset fields whichever base is selected -- a base of its own per
// slot would cost a scalar addition and a move into a vector register each).  Adding +0 is exact, so the sum is that of
// the plain loop, bit for bit.  The slot counts are facts about the band tables (group_band_fits, checked at run time on the
// real tables); the reads go out in batches of group_batch_pairs slots, all of a batch before the first wait.
#pragma once

constexpr int kGroupSpectrumBins = 776;              // the weighted spectrum Pw[0 .. 775] the kernel keeps in LDS: no band reaches beyond
constexpr int group_lanes(int nb) { return (nb + 1) / 2; }              // lanes with bands; the middle lane's two are one
constexpr bool group_band_is_wide(int nb, int band) { return band >= group_lanes(nb); }
// pair slots per band of the narrow / the wide half, by band count (109: basic version, 55: advanced)
constexpr int group_narrow_pairs(int nb) { return nb == 109 ? 1 : nb == 55 ? 3 : -1; }
constexpr int group_wide_pairs(int nb) { return nb == 109 ? 12 : nb == 55 ? 25 : -1; }
// wide pair slots whose reads are in flight together (their data registers: four per slot)
#ifdef PEAQ_FE_GROUP_BATCH
constexpr int group_batch_pairs(int nb) { return PEAQ_FE_GROUP_BATCH; }
#else
constexpr int group_batch_pairs(int nb) { return nb == 109 ? 4 : 5; }
#endif
constexpr int group_zero_words(int nb) { return 2 * group_wide_pairs(nb); }   // zero .. zero + this - 1 read as +0
constexpr int group_wide_batches(int nb) { return (group_wide_pairs(nb) + group_batch_pairs(nb) - 1) / group_batch_pairs(nb); }

// whole pairs among the interior bins lo + 1 .. hi - 1 (none for lo == hi and for adjacent edges)
constexpr int group_pairs(int lo, int hi) { return hi - lo - 1 > 0 ? (hi - lo - 1) >> 1 : 0; }
constexpr bool group_has_leftover(int lo, int hi) { return hi - lo - 1 > 0 && ((hi - lo - 1) & 1); }
// pair slot j of a band with `pairs` whole pairs fetches real bins
constexpr bool group_slot_live(int pairs, int j) { return j < pairs; }
// The reads of pair slot j are base + 2 j and base + 2 j + 1 (the constant part sits in the read's offset fields):
constexpr int group_slot_base(int lo, int pairs, int j, int zero) { return group_slot_live(pairs, j) ? lo + 1 : zero; }
constexpr int group_leftover_index(int lo, int hi, int zero) { return group_has_leftover(lo, hi) ? hi - 1 : zero; }

// a band of the tables fits the slots of its half
constexpr bool group_band_fits(int nb, int band, int lo, int hi) {
  return lo >= 0 && hi >= lo && group_pairs(lo, hi) <= (group_band_is_wide(nb, band) ? group_wide_pairs(nb) : group_narrow_pairs(nb));
}

// One band by the schedule, in plain C++ (the kernel's group_bands is this with the reads of a batch issued together):
// edge terms first, then the pair slots ascending, first element before second, the leftover bin last, then the floor.
template <typename T>
constexpr T group_band_scheduled(int slots, int lo, int hi, T wlo, T whi, const T* sp, int zero) {
  const int pairs = group_pairs(lo, hi);
  T p = wlo * sp[lo] + whi * sp[hi];
  for (int j = 0; j < slots; ++j) {
    const int base = group_slot_base(lo, pairs, j, zero);
    p += sp[base + 2 * j];
    p += sp[base + 2 * j + 1];
  }
  p += sp[group_leftover_index(lo, hi, zero)];
  return p < 1e-12 ? 1e-12 : p;
}

#ifndef PEAQ_FE_GROUP_BATCH
static_assert(group_wide_batches(109) == 3 && group_wide_batches(55) == 5, "three / five round trips for the wide band");
#endif
static_assert(group_pairs(5, 5) == 0 && group_pairs(5, 6) == 0 && group_pairs(5, 7) == 0 && !group_has_leftover(5, 6) &&
                  group_has_leftover(5, 7) && group_pairs(5, 8) == 1 && !group_has_leftover(5, 8) && group_pairs(5, 31) == 12 &&
                  group_has_leftover(5, 31),
              "pairs and leftover of a band");
