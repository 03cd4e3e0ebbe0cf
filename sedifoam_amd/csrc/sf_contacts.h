// sf_contacts.h -- `compute ID group pair/local v...` (the reference's name: gran/local) and the rows behind
// `dump ID group local N file col...` and sf_lammps_get_contacts (sf_contacts.hip): one row per touching pair, evaluated on
// the GPU from the state at the moment of the output.  The ID space, `compute` and `uncompute` are sf_compute_ids.h's; this
// kind plugs in there as pair_local_kind().
#pragma once
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

namespace sf {
struct SfLammps;

// the values of a row ([3P] compute pair/local names, plus the reference's tag1 tag2).  The first kContactDoubles are the
// double columns of ContactRows::val, in this order
enum ContactValue : unsigned char {
  CV_DIST, CV_FORCE, CV_FX, CV_FY, CV_FZ, CV_P1, CV_P2, CV_P3, CV_P4, CV_ENG, CV_TAG1, CV_TAG2, CV_COUNT
};
constexpr int kContactDoubles = 9;
constexpr unsigned char kContactIndex = 255;   // dump local's `index` column (the row number, 1-based)
constexpr int kContactMaxCols = 64;

// the rows of one evaluation, field-major on the device; valid until the next evaluation of the same engine
struct ContactRows {
  long long n = 0;
  const int* tag1 = nullptr;   // [n] the lower tag of the pair: the row's forces are those on it
  const int* tag2 = nullptr;   // [n]
  const double* val = nullptr; // [kContactDoubles][n]
};

struct ContactCols {   // the columns of a text line: ContactValue or kContactIndex
  int n;
  unsigned char c[kContactMaxCols];
};

// the values and the group of compute pair/local `id` (fails with LAMMPS' wording when there is none)
void compute_lookup(const SfLammps& L, const std::string& id, std::vector<unsigned char>* values, int* groupbit);
// count + scan + rows on the engine's stream; synchronises it once (the row count).  ms != nullptr: the GPU time of the
// three launches from HIP events (the wait for the count lies between two pairs of events and is not in it)
ContactRows contact_rows(SfLammps& L, int groupbit, double* ms = nullptr);
// k_contact_lines: the "%d " / "%g " of the columns `cols` of every row and "\n" into slots of `stride` bytes, and the lengths
void contact_lines_launch(const ContactRows& R, const ContactCols& cols, int stride, char* slots, unsigned long long* len,
                          hipStream_t s);
int contact_line_stride(const ContactCols& cols);
long long contact_launches(const SfLammps& L);

// sf_dump.hip: does a dump name this compute (a dump local its pair/local, a dump custom a per-atom compute)?
bool dump_uses_compute(const SfLammps& L, const std::string& id);
// sf_dump.hip (tools/contact_cost.py): every column of every row as text through the dump pipeline, nothing written;
// returns the byte count and the GPU time of lines + scan + compact
size_t dump_local_cost(SfLammps& L, const ContactRows& R, double* ms);
}  // namespace sf
