// list_policy_check.cpp -- csrc/sf_list_policy.h as a stand-alone program for the host sanitizers (tests/test_list_policy.py
// builds it with -fsanitize=address,undefined and runs it once).  The reference is the engine's spelling of every rule from
// before the header existed -- the if / else if ladders of bin_and_build, choose_kernel and list_stats_near_a_threshold
// with their literals, written out below as they stood -- and the header must take the same decision for every state, pin
// and fraction tried.  Prints one line per failure and the count; exit status 0 when there is none.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../sedifoam_amd/csrc/sf_list_policy.h"

namespace {
int failures = 0, checks = 0;

void expect(bool ok, const char* what, double frac, int state, int pin)
{
  checks++;
  if (ok) return;
  if (failures < 40) std::printf("FAIL %s: frac %.17g state %d pin %d\n", what, frac, state, pin);
  failures++;
}

// ---- the reference: the ladders as the engine spelled them.  `measured` stands for "slots > 0", frac for the quotient ----

bool ref_hist_single(bool hist_single_, int hist_mode_env_, bool roots_, bool have_list_, bool measured, double frac)
{
  if (hist_mode_env_ == 1) hist_single_ = true;
  else if (hist_mode_env_ == 2 || !roots_) hist_single_ = false;
  else if (have_list_ && measured) {
    if (hist_single_ && frac < 0.45) hist_single_ = false;
    else if (!hist_single_ && frac > 0.60) hist_single_ = true;
  }
  return hist_single_;
}

bool ref_touch_first(bool touch_first_, int touch_first_env_, bool have_list_, bool measured, double frac)
{
  if (touch_first_env_ >= 0) touch_first_ = touch_first_env_ != 0;
  else if (have_list_ && measured) {
    if (!touch_first_ && frac < 0.40) touch_first_ = true;
    else if (touch_first_ && frac > 0.50) touch_first_ = false;
  }
  return touch_first_;
}

int ref_sort_sub(int sort_sub_, long long nbuilds_, bool measured, double f)
{
  if (measured && nbuilds_ >= 2) {
    if (f < 0.70) sort_sub_ = 1;
    else if (f > 0.85) sort_sub_ = 2;
  }
  return sort_sub_;
}

bool ref_touch_prefetch(bool touch_prefetch_, int touch_prefetch_env_, bool measured, double frac)
{
  if (touch_prefetch_env_ >= 0) {
    touch_prefetch_ = touch_prefetch_env_ != 0;
    return touch_prefetch_;
  }
  if (!measured) return touch_prefetch_;
  if (touch_prefetch_ && frac > 0.85) touch_prefetch_ = false;
  else if (!touch_prefetch_ && frac < 0.70) touch_prefetch_ = true;
  return touch_prefetch_;
}

bool ref_near(bool part_measured, double c, bool list_measured, double t)
{
  const double m = 0.08;
  if (part_measured) {
    if (c > 0.45 - m && c < 0.60 + m) return true;
  }
  if (list_measured) {
    if ((t > 0.40 - m && t < 0.50 + m) || (t > 0.70 - m && t < 0.85 + m)) return true;
  }
  return false;
}

bool ref_measure(long long nbuilds_, bool near) { return nbuilds_ < 4 || (nbuilds_ & 3) == 0 || near; }

int ref_nt_policy(int nlocal_, long long list_sampled_, int list_slots, bool hist_single_, int nt_policy_env_)
{
  const double khalf = (list_sampled_ > 0 && list_slots > 0) ? 0.5 * (double)list_slots / (double)list_sampled_ : 6.0;
  const double copies = hist_single_ ? 1.0 : 2.0;
  const double touched = (double)nlocal_ * (252.0 + (8.0 + 48.0 * copies) * khalf);
  const double mall = 256.0 * 1024.0 * 1024.0;
  int nt_policy_;
  if (nt_policy_env_ >= 0) nt_policy_ = nt_policy_env_;
  else if (touched < mall) nt_policy_ = 0;
  else if (touched < 1.4 * mall) nt_policy_ = 3;
  else nt_policy_ = hist_single_ ? 1 : 2;
  return nt_policy_;
}

// ---- the fractions: the sweep, every band edge and every near-a-band edge with the doubles on both sides ----

void with_neighbours(std::vector<double>& v, double x)
{
  v.push_back(std::nextafter(x, -1.0));
  v.push_back(x);
  v.push_back(std::nextafter(x, 2.0));
}

std::vector<double> fractions()
{
  std::vector<double> v;
  for (int k = 0; k <= 1000; k++) v.push_back(k / 1000.0);
  for (double edge : {0.40, 0.45, 0.50, 0.60, 0.70, 0.85}) with_neighbours(v, edge);
  const double m = 0.08;   // (0.32, 0.37, 0.58, 0.62, 0.68, 0.93 as the engine computes them)
  for (double edge : {0.40 - m, 0.45 - m, 0.50 + m, 0.70 - m, 0.60 + m, 0.85 + m}) with_neighbours(v, edge);
  return v;
}

sf::ListStats stats(bool part_measured, double c, bool list_measured, double t)
{
  return sf::ListStats{part_measured, c, list_measured, t};
}

void check_decisions(const std::vector<double>& fr)
{
  for (double f : fr)
    for (int measured = 0; measured < 2; measured++) {
      const sf::ListStats s = stats(measured, f, measured, f);
      for (int have_list = 0; have_list < 2; have_list++)
        for (int state = 0; state < 2; state++) {
          for (int pin = 0; pin <= 2; pin++)
            for (int roots = 0; roots < 2; roots++)
              expect(sf::choose_hist_single(state, s, have_list, pin, roots) ==
                         ref_hist_single(state, pin, roots, have_list, measured, f), "hist_single", f, state, pin);
          for (int pin = -1; pin <= 1; pin++)
            expect(sf::choose_touch_first(state, s, have_list, pin) == ref_touch_first(state, pin, have_list, measured, f),
                   "touch_first", f, state, pin);
        }
      for (int state = 0; state < 2; state++)
        for (int pin = -1; pin <= 1; pin++)
          expect(sf::choose_touch_prefetch(state, s, pin) == ref_touch_prefetch(state, pin, measured, f), "touch_prefetch", f,
                 state, pin);
      for (int state = 0; state <= 2; state++)
        for (long long nbuilds = 0; nbuilds <= 3; nbuilds++)
          expect(sf::choose_sort_sub(state, s, nbuilds) == ref_sort_sub(state, nbuilds, measured, f), "sort_sub", f, state,
                 (int)nbuilds);
    }
}

void check_counters()
{
  // the fractions as the engine forms them: (double)a / (double)b of two counters; nothing counted = not measured
  for (int slots : {0, 1, 3, 7, 1000, 123457})
    for (int k = 0; k <= 20; k++) {
      const int part = (int)((long long)slots * k / 20);
      const sf::ListStats s = sf::ListStats::from_counters(slots, part, slots, part);
      expect(s.has_coalescing == (slots > 0) && s.has_touching == (slots > 0), "from_counters: measured", k / 20.0, slots, 0);
      if (slots > 0)
        expect(s.coalescing == (double)part / (double)slots && s.touching == (double)part / (double)slots,
               "from_counters: quotient", k / 20.0, slots, 0);
    }
  const sf::ListStats one = sf::ListStats::from_counters(0, 5, 10, 4);
  expect(!one.has_coalescing && one.has_touching && one.touching == 4.0 / 10.0, "from_counters: one of two", 0.4, 0, 0);
}

void check_near_and_schedule(const std::vector<double>& fr)
{
  for (double f : fr)
    for (int pm = 0; pm < 2; pm++)
      for (int lm = 0; lm < 2; lm++) {
        // each fraction on its own (the other far from every band) and both together
        expect(sf::stats_near_a_band(stats(pm, f, lm, 0.0)) == ref_near(pm, f, lm, 0.0), "near: coalescing", f, pm, lm);
        expect(sf::stats_near_a_band(stats(pm, 0.0, lm, f)) == ref_near(pm, 0.0, lm, f), "near: touching", f, pm, lm);
        expect(sf::stats_near_a_band(stats(pm, f, lm, f)) == ref_near(pm, f, lm, f), "near: both", f, pm, lm);
      }
  for (long long nbuilds = 0; nbuilds <= 16; nbuilds++)
    for (int near = 0; near < 2; near++)
      expect(sf::measure_this_list(nbuilds, near) == ref_measure(nbuilds, near), "measure schedule", 0.0, (int)nbuilds, near);
}

void check_nt_policy()
{
  const double mall = 256.0 * 1024.0 * 1024.0;
  for (int single = 0; single < 2; single++)
    for (long long sampled : {0LL, 1024LL, 65536LL})
      for (int khalf2 : {0, 9, 12, 15}) {   // listed neighbours per sampled atom (twice K_half); 0: not measured
        const int list_slots = (int)(sampled * khalf2);
        const double khalf = (sampled > 0 && list_slots > 0) ? 0.5 * khalf2 : 6.0;
        const double per_atom = 252.0 + (8.0 + 48.0 * (single ? 1.0 : 2.0)) * khalf;
        for (double bound : {mall, 1.4 * mall}) {
          const int n0 = (int)(bound / per_atom);   // the atom counts around the one whose bytes cross the bound
          for (int nlocal = n0 - 2; nlocal <= n0 + 2; nlocal++)
            for (int pin = -1; pin <= 3; pin++) {
              const double touched = sf::substep_bytes_touched(nlocal, sampled, list_slots, single);
              expect(sf::choose_nt_policy(touched, single, pin) == ref_nt_policy(nlocal, sampled, list_slots, single, pin),
                     "nt_policy", touched / mall, single, pin);
            }
          // (the sweep above does see both sides of the bound)
          expect(sf::substep_bytes_touched(n0 - 2, sampled, list_slots, single) < bound &&
                     sf::substep_bytes_touched(n0 + 2, sampled, list_slots, single) > bound, "nt_policy: bound straddled",
                 bound / mall, single, khalf2);
        }
        // (slots counted but no atom sampled: K_half falls back to 6 all the same)
        expect(sf::substep_bytes_touched(500000, 0, 5000, single) == 500000.0 * (252.0 + (8.0 + 48.0 * (single ? 1.0 : 2.0)) * 6.0),
               "nt_policy: no sample", 0.0, single, 0);
        for (int nlocal : {0, 1, 1000, 100000, 1000000, 4000000})
          expect(sf::choose_nt_policy(sf::substep_bytes_touched(nlocal, sampled, list_slots, single), single, -1) ==
                     ref_nt_policy(nlocal, sampled, list_slots, single, -1), "nt_policy: sizes", (double)nlocal, single, -1);
      }
}

// a fraction drifting up through each band and down again, one list after another: the states carried along by the header
// and by the ladders stay equal step by step, and each switches once per crossing
void check_drift()
{
  std::vector<double> walk;
  for (int k = 300; k <= 950; k += 5) walk.push_back(k / 1000.0);
  for (int k = 950; k >= 300; k -= 5) walk.push_back(k / 1000.0);
  bool hs = true, hs_ref = true, tf = false, tf_ref = false, tp = true, tp_ref = true;
  int sub = 0, sub_ref = 0, switches = 0;
  long long nbuilds = 0;
  for (double f : walk) {
    const sf::ListStats s = stats(true, f, true, f);
    const bool hs0 = hs, tf0 = tf, tp0 = tp;
    const int sub0 = sub;
    hs = sf::choose_hist_single(hs, s, true, 0, true);
    hs_ref = ref_hist_single(hs_ref, 0, true, true, true, f);
    tf = sf::choose_touch_first(tf, s, true, -1);
    tf_ref = ref_touch_first(tf_ref, -1, true, true, f);
    tp = sf::choose_touch_prefetch(tp, s, -1);
    tp_ref = ref_touch_prefetch(tp_ref, -1, true, f);
    sub = sf::choose_sort_sub(sub, s, nbuilds);
    sub_ref = ref_sort_sub(sub_ref, nbuilds, true, f);
    nbuilds++;
    expect(hs == hs_ref && tf == tf_ref && tp == tp_ref && sub == sub_ref, "drift", f, hs * 8 + tf * 4 + tp * 2, sub);
    switches += (hs != hs0) + (tf != tf0) + (tp != tp0) + (sub != sub0 && sub0 != 0);
  }
  // up: hist_single and touch_first each switch once at most, prefetch and sort cells once; down: each once again.  hs starts
  // true below its band (switches to false at once), tf starts false below its band (true at once)
  expect(switches == 10, "drift: switches per cycle", (double)switches, 0, 0);
}
}  // namespace

int main()
{
  const std::vector<double> fr = fractions();
  check_decisions(fr);
  check_counters();
  check_near_and_schedule(fr);
  check_nt_policy();
  check_drift();
  std::printf("%d checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
