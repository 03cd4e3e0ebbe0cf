// ave_common_check.cpp -- csrc/sf_ave_common.h as a stand-alone program for the host sanitizers (tests/test_ave_common.py
// builds it with -fsanitize=address,undefined and runs it once in a scratch directory, given as argv[1]): the schedule
// against a brute-force statement of the LAMMPS rule, the output file, the shared keywords, and the one c_ID[k] parser through
// the dump column of csrc/sf_compute_parse.h.  Prints one line per failure; exit status 0 when there is none.
#include <cstdio>
#include <fstream>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "../../sedifoam_amd/csrc/sf_compute_parse.h"

namespace {
int failures = 0, checks = 0;

void expect(bool ok, const std::string& what)
{
  checks++;
  if (ok) return;
  std::printf("FAIL %s\n", what.c_str());
  failures++;
}

// ---- the schedule ----

// The rule, stated without the arithmetic of ave_first_valid.  An output belongs to every multiple M of Nfreq from the
// first one on; its samples are the steps M - j Nevery, 0 <= j < Nrepeat.  The first output of a fix defined at step t0 is
// the least multiple M of Nfreq with M > t0 and M >= start whose samples all lie at or after t0 -- except that with
// Nrepeat = 1 a fix defined on a multiple of Nfreq samples (and puts out) at once, at t0 itself, unless `start` lies beyond
// the next multiple ([3P] FixAveTime::nextvalid tests `start` against that next multiple, not against t0)
struct Brute {
  std::set<long long> samples, outputs;
  Brute(long nevery, long nrepeat, long nfreq, long start, long long t0, long long horizon)
  {
    long long M = 0;
    if (nrepeat == 1 && t0 % nfreq == 0 && start <= t0 + nfreq) M = t0;
    else {
      M = nfreq;
      while (!(M > t0 && M >= start && M - (nrepeat - 1) * nevery >= t0)) M += nfreq;
    }
    for (; M - (nrepeat - 1) * nevery <= horizon; M += nfreq) {
      outputs.insert(M);
      for (long j = 0; j < nrepeat; j++) samples.insert(M - j * nevery);
    }
  }
  long long next_after(long long step) const { return *samples.upper_bound(step); }
};

// S walks the steps t0 .. t1 as run_steps would (every step visited) and must agree with the rule for a fix defined at t0
bool walk(sf::AveSchedule& S, const Brute& B, long long t0, long long t1)
{
  bool ok = true;
  for (long long s = t0; s <= t1; s++) {
    ok = ok && !S.catch_up(s);   // (no step was skipped)
    const bool due = S.due(s);
    ok = ok && due == (B.samples.count(s) == 1);
    if (due) ok = ok && S.sampled(s) == (B.outputs.count(s) == 1);
    ok = ok && S.next(s) == B.next_after(s);
  }
  return ok;
}

void schedules()
{
  const long starts[3] = {0, 7, 20};
  int accepted = 0;
  for (long nfreq = 1; nfreq <= 12; nfreq++)
    for (long nevery = 1; nevery <= 13; nevery++)
      for (long nrepeat = 1; nrepeat <= 13; nrepeat++) {
        sf::AveSchedule P;
        const std::vector<std::string> w = {std::to_string(nevery), std::to_string(nrepeat), std::to_string(nfreq)};
        const bool legal = nfreq % nevery == 0 && nrepeat * nevery <= nfreq;
        const std::string tag = w[0] + " " + w[1] + " " + w[2];
        const std::string err = P.parse(w, 0, "Illegal x");
        expect(err == (legal ? "" : "Illegal x"), "parse " + tag);
        if (!err.empty()) continue;
        accepted++;
        for (long start : starts)
          for (long long t0 = 0; t0 <= 25; t0++) {
            const long long horizon = t0 + 4 * nfreq + 40;
            const std::string at = tag + " start " + std::to_string(start) + " t0 " + std::to_string(t0);
            sf::AveSchedule S = P;
            S.start = start;
            S.begin(t0);
            const Brute B(nevery, nrepeat, nfreq, start, t0, horizon + 2 * nfreq + 40);
            expect(S.nvalid == sf::ave_first_valid(t0, nevery, nrepeat, nfreq, start), "begin " + at);
            expect(walk(S, B, t0, horizon), "walk " + at);
            // steps skipped in the middle of an output: stop after the first sample of a block of several, jump ahead
            if (nrepeat < 2) continue;
            for (long long skip = 1; skip <= 15; skip++) {
              sf::AveSchedule C = P;
              C.start = start;
              C.begin(t0);
              const long long first = C.nvalid;
              bool ok = !C.sampled(first) && C.irepeat == 1;   // (one sample taken; the next is due at first + nevery)
              const long long now = first + skip;
              const bool missed = now > first + nevery;
              const long long next_before = C.next(now - 1);
              ok = ok && C.catch_up(now) == missed;
              if (missed) {   // a fix defined at `now`, with nothing accumulated
                const Brute R(nevery, nrepeat, nfreq, start, now, now + 6 * nfreq + 80);
                ok = ok && next_before == *R.samples.begin() && C.irepeat == 0 && walk(C, R, now, now + 3 * nfreq + 40);
              } else {        // nothing happened: the output under way goes on
                ok = ok && C.irepeat == 1 && C.nvalid == first + nevery && walk(C, B, now, horizon);
              }
              expect(ok, "catch_up after " + std::to_string(skip) + " steps, " + at);
            }
          }
      }
  // (Nevery divides Nfreq and Nrepeat <= Nfreq / Nevery: the sum of the divisor sums of 1 .. 12)
  expect(accepted == 127, "the schedules with Nfreq <= 12 that the parser accepts: " + std::to_string(accepted));
  sf::AveSchedule P;
  expect(P.parse({"2", "3"}, 0, "I") == "I" && P.parse({"0", "1", "10"}, 0, "I") == "I" && P.parse({"2", "x", "10"}, 0, "I") == "I" &&
             P.parse({"a", "b", "2", "3", "10"}, 2, "I").empty() && P.nevery == 2 && P.nrepeat == 3 && P.nfreq == 10,
         "parse: missing, zero and non-numeric words, and an offset");
}

// ---- the file ----

std::string slurp(const std::string& path)
{
  std::ifstream f(path, std::ios::binary);
  std::ostringstream o;
  o << f.rdbuf();
  return o.str();
}

// three outputs; the second is longer than the third
std::string three_blocks(sf::AveFile& F)
{
  const char* const body[3] = {"10 a\n", "20 a much longer block\n  with two lines\n", "30 b\n"};
  std::string err;
  for (int k = 0; k < 3 && err.empty(); k++) {
    err = F.begin_block();
    fputs(body[k], F.fp());
    if (err.empty()) err = F.end_block();
  }
  return err;
}

void files(const std::string& dir)
{
  const std::string defaults[3] = {"# one", "# two", "# three"};
  const std::string all = "10 a\n20 a much longer block\n  with two lines\n30 b\n";
  {
    sf::AveFile F;
    expect(F.open(sf::AveFileSpec(), "ave/time", "t", defaults, 2).empty() && F.fp() == nullptr, "no file keyword: no file");
  }
  {
    sf::AveFileSpec S;
    S.file = dir + "/append.txt";
    sf::AveFile F;
    expect(F.open(S, "ave/chunk", "p", defaults, 3).empty() && F.fp() != nullptr, "open");
    expect(slurp(S.file) == "# one\n# two\n# three\n", "default titles are on disk once the file is open");
    expect(three_blocks(F).empty() && slurp(S.file) == "# one\n# two\n# three\n" + all, "three outputs appended");
  }
  {
    sf::AveFileSpec S;
    S.file = dir + "/titles.txt";
    S.has_title[0] = S.has_title[2] = true;
    S.title[0] = "my first";
    S.title[2] = "";
    sf::AveFile F;
    expect(F.open(S, "ave/histo", "h", defaults, 3).empty() && slurp(S.file) == "my first\n# two\n\n", "given titles, an empty one too");
    sf::AveFile G;
    S.file = dir + "/two.txt";
    expect(G.open(S, "ave/time", "t", defaults, 2).empty() && slurp(S.file) == "my first\n# two\n", "two title lines");
  }
  {
    sf::AveFileSpec S;
    S.file = dir + "/over.txt";
    S.overwrite = true;
    sf::AveFile F;
    expect(F.open(S, "ave/chunk", "p", defaults, 3).empty(), "open with overwrite");
    std::string err = F.begin_block();
    fputs("20 a much longer block\n  with two lines\n", F.fp());
    err += F.end_block();
    expect(err.empty() && slurp(S.file) == "# one\n# two\n# three\n20 a much longer block\n  with two lines\n", "overwrite: one block");
    expect(three_blocks(F).empty() && slurp(S.file) == "# one\n# two\n# three\n30 b\n", "overwrite: the last block alone, truncated");
  }
  {
    sf::AveFileSpec S;
    S.file = dir + "/no/such/dir/f.txt";
    sf::AveFile F;
    expect(F.open(S, "ave/histo", "h", defaults, 3) == "Cannot open fix ave/histo file " + S.file && F.fp() == nullptr, "an unwritable path");
  }
}

// ---- the keywords and the c_ID[k] word ----

void keywords()
{
  const std::vector<std::string> w = {"file", "f.txt", "overwrite", "title2", "a b", "ave", "window", "4", "start", "30", "norm", "title1"};
  sf::AveFileSpec F;
  int ave = sf::AVE_ONE;
  long window = 0, start = 0;
  size_t k = 0;
  bool ok = sf::ave_file_keyword(w, &k, &F) == sf::AK_CONSUMED && k == 2 && sf::ave_file_keyword(w, &k, &F) == sf::AK_CONSUMED && k == 3 &&
            sf::ave_file_keyword(w, &k, &F) == sf::AK_CONSUMED && k == 5 && sf::ave_file_keyword(w, &k, &F) == sf::AK_NOT_MINE && k == 5;
  ok = ok && F.file == "f.txt" && F.overwrite && !F.has_title[0] && F.has_title[1] && F.title[1] == "a b";
  ok = ok && sf::ave_mode_keyword(w, &k, &ave, &window, &start) == sf::AK_CONSUMED && k == 8 && ave == sf::AVE_WINDOW && window == 4;
  ok = ok && sf::ave_mode_keyword(w, &k, &ave, &window, &start) == sf::AK_CONSUMED && k == 10 && start == 30;
  ok = ok && sf::ave_mode_keyword(w, &k, &ave, &window, &start) == sf::AK_NOT_MINE && sf::ave_file_keyword(w, &k, &F) == sf::AK_NOT_MINE && k == 10;
  k = 11;   // (a keyword without its word, at the end of the line)
  ok = ok && sf::ave_file_keyword(w, &k, &F) == sf::AK_ERROR;
  expect(ok, "file, overwrite, title, ave and start keywords");
  for (const std::vector<std::string>& bad : std::vector<std::vector<std::string>>{
           {"ave"}, {"ave", "window"}, {"ave", "window", "0"}, {"ave", "window", "x"}, {"ave", "sometimes"}, {"start"}, {"start", "-1"}, {"file", ""}}) {
    k = 0;
    sf::AveKey r = sf::ave_file_keyword(bad, &k, &F);
    if (r == sf::AK_NOT_MINE) r = sf::ave_mode_keyword(bad, &k, &ave, &window, &start);
    expect(r == sf::AK_ERROR && k == 0, "refused: " + bad[0] + (bad.size() > 1 ? " " + bad[1] : ""));
  }
  expect(sf::ave_attr_of("x") == sf::AA_X && sf::ave_attr_of("vz") == sf::AA_VZ && sf::ave_attr_of("fz") == sf::AA_FZ &&
             sf::ave_attr_of("density/mass") < 0 && sf::ave_attr_of("") < 0,
         "attribute words");
}

void crefs()
{
  std::string id;
  long index = -1;
  expect(sf::parse_cref("c_s", &id, &index) && id == "s" && index == 0, "c_s");
  expect(sf::parse_cref("c_st[6]", &id, &index) && id == "st" && index == 6, "c_st[6]");
  expect(sf::parse_cref("c_s[1000000]", &id, &index) && index == 1000000, "c_s[1000000]");
  for (const char* bad : {"", "c_", "s", "v_s", "c_[2]", "c_s[", "c_s[]", "c_s]", "c_s[0]", "c_s[-1]", "c_s[+1]", "c_s[ 1]", "c_s[1 ]", "c_s[1]x",
                          "c_s[1][2]", "c_s[x]", "c_s[1000001]", "c_s[99999999999999999999]", "c_s[*]"})
    expect(!sf::parse_cref(bad, &id, &index), std::string("refused: ") + bad);
  // a dump column: the same words, with the text of the dump command
  expect(sf::parse_compute_column("c_s[4]", "custom", &id, &index).empty() && id == "s" && index == 4, "dump column c_s[4]");
  for (const char* bad : {"c_s[+1]", "c_s[ 1]", "c_s]", "c_s[1000001]", "c_s[0]", "c_s[2"})
    expect(sf::parse_compute_column(bad, "custom", &id, &index) == std::string("Invalid attribute ") + bad + " in dump custom command",
           std::string("dump column refused: ") + bad);
}
}  // namespace

int main(int argc, char** argv)
{
  if (argc != 2) {
    std::printf("usage: ave_common_check SCRATCH_DIRECTORY\n");
    return 2;
  }
  schedules();
  files(argv[1]);
  keywords();
  crefs();
  std::printf("%d checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
