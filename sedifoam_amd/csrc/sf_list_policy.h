// sf_list_policy.h -- every rule that turns the statistics of a neighbour list into a choice, each written once.  Host only,
// no HIP headers, no environment: the pins of the SF_* knobs enter as plain arguments (the engine's constructor reads them).
//
// The statistics are four counters that k_partner_coalescing leaves in the flag words (DemEngine::measure_list); two
// fractions are taken from them.  Each choice sits behind a hysteresis band on one fraction:
//
//   fraction                    band          user (DemEngine)   below lo        above hi
//   coalescing of partner sides 0.45 / 0.60   hist_single_       false (two)     true (one history copy)
//   listed neighbours touching  0.40 / 0.50   touch_first_       true            false
//   listed neighbours touching  0.70 / 0.85   touch_prefetch_    true            false
//   listed neighbours touching  0.70 / 0.85   sort_sub_          1 (full cells)  2 (half-cutoff cells)
//
// Inside a band (edges included: every comparison is strict) the state stays.  A list is measured on the first four
// builds, on every fourth one, and whenever a fraction lies within kNearMargin of a band -- so the decisions are those of
// measuring EVERY list as long as a fraction does not jump a whole margin between two lists.
#pragma once

namespace sf {

struct Band {
  double lo, hi;
  // the state after a measurement `frac`: `below` under lo, `above` over hi, unchanged in between
  template <class T>
  T step(T state, double frac, T below, T above) const { return frac < lo ? below : frac > hi ? above : state; }
  // could the next measurement switch a state?  (the open interval lo - margin .. hi + margin)
  bool near(double frac, double margin) const { return frac > lo - margin && frac < hi + margin; }
};

constexpr Band kHistCopiesBand{0.45, 0.60};   // partner-side coalescing: history copies
constexpr Band kTouchFirstBand{0.40, 0.50};   // touching fraction: slot order of a row
constexpr Band kTouchDenseBand{0.70, 0.85};   // touching fraction: v, omega prefetch and the size of the sort cells
constexpr double kNearMargin = 0.08;

// the two fractions of the last measured list, from its counters (F_PART_SLOTS, F_PART_COAL, F_LIST_SLOTS, F_LIST_TOUCH);
// no slots counted: not measured, the fraction is not looked at
struct ListStats {
  bool has_coalescing;
  double coalescing;   // would-be partner-side gathers that coalesce / all of them
  bool has_touching;
  double touching;     // listed neighbours that touch / all of them
  static ListStats from_counters(int part_slots, int part_coal, int list_slots, int list_touch)
  {
    return ListStats{part_slots > 0, part_slots > 0 ? (double)part_coal / (double)part_slots : 0.0,
                     list_slots > 0, list_slots > 0 ? (double)list_touch / (double)list_slots : 0.0};
  }
};

// SF_HIST_COPIES = 1 / 2 pins the copies; words that are not (root, image code) always keep two
inline bool hist_copies_pinned(int pin, bool roots) { return pin == 1 || pin == 2 || !roots; }

// one history copy per contact (true) or one per side (false) for the list about to be built; the first list is built
// with the state it is given
inline bool choose_hist_single(bool state, const ListStats& s, bool have_list, int pin, bool roots)
{
  if (pin == 1) return true;
  if (hist_copies_pinned(pin, roots)) return false;
  if (!have_list || !s.has_coalescing) return state;
  return kHistCopiesBand.step(state, s.coalescing, false, true);
}

// touching neighbours in the first slots of a row (SF_TOUCH_FIRST = 0 / 1 pins it, -1: by the statistics)
inline bool choose_touch_first(bool state, const ListStats& s, bool have_list, int pin)
{
  if (pin >= 0) return pin != 0;
  if (!have_list || !s.has_touching) return state;
  return kTouchFirstBand.step(state, s.touching, true, false);
}

// v, omega of a neighbour prefetched by touch bit (SF_TOUCH_PREFETCH = 0 / 1 pins it, -1: by the statistics)
inline bool choose_touch_prefetch(bool state, const ListStats& s, int pin)
{
  if (pin >= 0) return pin != 0;
  if (!s.has_touching) return state;
  return kTouchDenseBand.step(state, s.touching, true, false);
}

// sort cells per cutoff length, from the second list on (the first list of a run carries no touch bits)
inline int choose_sort_sub(int state, const ListStats& s, long long nbuilds)
{
  if (!s.has_touching || nbuilds < 2) return state;
  return kTouchDenseBand.step(state, s.touching, 1, 2);
}

// true when a decision above could change with the next measurement
inline bool stats_near_a_band(const ListStats& s)
{
  const double m = kNearMargin;
  if (s.has_coalescing && kHistCopiesBand.near(s.coalescing, m)) return true;
  if (s.has_touching && (kTouchFirstBand.near(s.touching, m) || kTouchDenseBand.near(s.touching, m))) return true;
  return false;
}

// is list number `nbuilds` (0 = the first) measured?
inline bool measure_this_list(long long nbuilds, bool near_a_band) { return nbuilds < 4 || (nbuilds & 3) == 0 || near_a_band; }

// Bytes one sub-step touches: records in + out 192 B, history in + out 48 B per stored copy, list words, fix arrays; half
// the listed neighbours per atom from the last measurement -- list_slots (F_LIST_SLOTS) over the list_sampled atoms it
// looked at --, 6 before there is one
inline double substep_bytes_touched(int nlocal, long long list_sampled, int list_slots, bool hist_single)
{
  const double khalf = (list_sampled > 0 && list_slots > 0) ? 0.5 * (double)list_slots / (double)list_sampled : 6.0;
  const double copies = hist_single ? 1.0 : 2.0;
  return (double)nlocal * (252.0 + (8.0 + 48.0 * copies) * khalf);
}

// Non-temporal policy of the row streams (sf_dem_kernels.h, NTP) from those bytes against the 256 MB memory-side cache
// (SF_NT_POLICY = 0 .. 3 pins it, -1: by size)
inline int choose_nt_policy(double touched, bool hist_single, int pin)
{
  const double mall = 256.0 * 1024.0 * 1024.0;
  if (pin >= 0) return pin;
  if (touched < mall) return 0;
  if (touched < 1.4 * mall) return 3;
  return hist_single ? 1 : 2;
}

}  // namespace sf
