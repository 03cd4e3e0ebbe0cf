// sf_pchunk_parse.h -- the words of `compute ID group chunk/atom c_CID | c_CID[k] [keywords]`, a chunk/atom compute whose
// chunk ID is a column of a per-atom compute, and of the four per-chunk computes `compute ID group property/chunk | com/chunk |
// vcm/chunk | gyration/chunk CHUNKID ...` ([3P] LAMMPS names and rules: ComputeChunkAtom, ComputePropertyChunk,
// ComputeCOMChunk, ComputeVCMChunk, ComputeGyrationChunk).  Host only, with nothing but the standard
// library, so that this code can be compiled into a stand-alone program and run under the host sanitizers
// (tests/c_abi/pchunk_parse_check.cpp).  Every parser returns an empty string, or the error text, and leaves the caller's
// spec alone when it refuses.  sf_chunk_parse.h goes on parsing the bin styles and refusing the others.
#pragma once
#include <string>
#include <vector>

#include "sf_ave_common.h"
#include "sf_compute_ref.h"

namespace sf {

// ---- compute chunk/atom c_CID ----

struct ChunkRefSpec {
  std::string cid;          // the per-atom compute the chunk ID is read from
  long index = 0;           // k of c_CID[k]; 0: c_CID, a one-column compute
  bool compress = false;    // the distinct IDs renumbered 1 .. Nchunk in ascending order
  bool nchunk_every = false;   // Nchunk is found at every evaluation (compress yes: always)
  bool rows_fixed() const { return !compress && !nchunk_every; }
};

// is word 4 of a compute chunk/atom line the new style?  (chunk_compute_define asks before it calls parse_chunk_atom)
inline bool chunk_style_is_compute(const std::vector<std::string>& w) { return w.size() > 4 && w[4].compare(0, 2, "c_") == 0; }

// w = compute ID group chunk/atom c_CID[k] [keywords]
inline std::string parse_chunk_atom_compute(const std::vector<std::string>& w, ChunkRefSpec* out)
{
  const std::string illegal = "Illegal compute chunk/atom command";
  if (w.size() < 5) return illegal;
  ChunkRefSpec S;
  if (!parse_cref(w[4], &S.cid, &S.index)) return illegal;
  int nchunk = -1;   // 0 once, 1 every, -1 not typed
  size_t k = 5;
  while (k < w.size()) {
    const std::string& key = w[k];
    const size_t left = w.size() - k - 1;
    if (key == "region")
      return "compute chunk/atom: region is not supported (give the compute a region group: group ID region RID, or group ID dynamic)";
    if (key == "bound" || key == "units")
      return "compute chunk/atom: " + key + " is not supported with " + w[4] + " (it belongs to the bin styles)";
    if (left < 1) return illegal;
    const std::string& v = w[k + 1];
    if (key == "nchunk") {
      if (v != "once" && v != "every") return illegal;
      nchunk = v == "every" ? 1 : 0;
    } else if (key == "compress") {
      if (v != "yes" && v != "no") return illegal;
      S.compress = v == "yes";
    } else if (key == "ids") {
      if (v == "once" || v == "nfreq")
        return "compute chunk/atom: ids " + v + " is not supported (ids every is: an atom is assigned anew at every sample)";
      if (v != "every") return illegal;
    } else if (key == "limit") {
      long lim = 0;
      if (!chunk_parse_int(v, &lim) || lim < 0) return illegal;
      if (lim > 0) return "compute chunk/atom: limit " + v + " is not supported (limit 0 is)";
    } else if (key == "discard") {
      if (v == "no" || v == "mixed")
        return "compute chunk/atom: discard " + v + " is not supported with " + w[4] + " (discard yes is: an ID above Nchunk gives chunk 0)";
      if (v != "yes") return illegal;
    } else if (key == "pbc") {
      if (v == "yes") return "compute chunk/atom: pbc yes is not supported (pbc no is)";
      if (v != "no") return illegal;
    } else
      return illegal;
    k += 2;
  }
  if (S.compress && nchunk == 0)
    return "compute chunk/atom: nchunk once is not supported with compress yes (the distinct IDs are found at every evaluation)";
  S.nchunk_every = S.compress || nchunk == 1;
  *out = S;
  return std::string();
}

// the column c_CID / c_CID[k] names (the wording of check_ave_chunk_value)
inline std::string check_chunk_atom_value(const ComputeShape& s, long index)
{
  if (s.kind == CK_NONE) return "Compute ID for compute chunk/atom does not exist";
  if (s.kind != CK_PERATOM) return "Compute chunk/atom compute does not calculate per-atom values";
  if (index == 0 && s.n != 1) return "Compute chunk/atom compute does not calculate a per-atom vector";
  if (index > 0 && s.n == 1) return "Compute chunk/atom compute does not calculate a per-atom array";
  if (index > s.n) return "Compute chunk/atom compute vector is accessed out-of-range";
  return std::string();
}

// ---- the per-chunk computes ----

enum PChunkStyle { PC_PROPERTY, PC_COM, PC_VCM, PC_GYRATION };
constexpr int kNumPChunkStyles = 4;
inline const char* pchunk_style_name(int style)
{
  static const char* const names[kNumPChunkStyles] = {"property/chunk", "com/chunk", "vcm/chunk", "gyration/chunk"};
  return names[style];
}
// PC_PROPERTY .. PC_GYRATION, or -1
inline int pchunk_style_of(const std::string& word)
{
  for (int s = 0; s < kNumPChunkStyles; s++)
    if (word == pchunk_style_name(s)) return s;
  return -1;
}

enum PChunkProp { PP_COUNT, PP_ID };
struct PChunkSpec {
  int style = PC_PROPERTY;
  std::string chunk;        // the ID of the chunk/atom compute
  std::vector<int> props;   // PC_PROPERTY: the columns, in the order typed
  bool tensor = false;      // PC_GYRATION: six columns xx yy zz xy xz yz
  int ncols() const
  {
    if (style == PC_PROPERTY) return (int)props.size();
    if (style == PC_GYRATION) return tensor ? 6 : 1;
    return 3;
  }
  bool wants_id() const
  {
    for (int p : props)
      if (p == PP_ID) return true;
    return false;
  }
};

// w = compute ID group STYLE CHUNKID ...
inline std::string parse_pchunk(const std::vector<std::string>& w, PChunkSpec* out)
{
  if (w.size() < 4) return "Illegal compute command";
  PChunkSpec S;
  S.style = pchunk_style_of(w[3]);
  if (S.style < 0) return "Illegal compute command";
  const std::string illegal = "Illegal compute " + w[3] + " command";
  if (w.size() < 5 || w[4].empty()) return illegal;
  if (w[4].compare(0, 2, "c_") == 0)
    return "compute " + w[3] + ": give the ID of the chunk/atom compute itself (" + w[4].substr(2) + ", not " + w[4] + ")";
  S.chunk = w[4];
  if (S.style == PC_PROPERTY) {
    if (w.size() < 6) return illegal;
    for (size_t k = 5; k < w.size(); k++) {
      if (w[k] == "count") S.props.push_back(PP_COUNT);
      else if (w[k] == "id") S.props.push_back(PP_ID);
      else if (w[k] == "coord1" || w[k] == "coord2" || w[k] == "coord3")
        return "compute property/chunk: " + w[k] + " is not supported (a chunk/atom compute over c_ID has no bins; count and id are)";
      else return illegal;
    }
  } else if (S.style == PC_GYRATION) {
    if (w.size() == 6 && w[5] == "tensor") S.tensor = true;
    else if (w.size() != 5) return illegal;
  } else if (w.size() != 5)
    return illegal;
  *out = S;
  return std::string();
}

// what CHUNKID must be; `compressed`: that chunk/atom compute has compress yes
inline std::string check_pchunk_chunk(const PChunkSpec& S, const ComputeShape& chunk, bool from_compute, bool compressed)
{
  const std::string who = std::string("compute ") + pchunk_style_name(S.style);
  if (chunk.kind == CK_NONE) return "Chunk/atom compute does not exist for " + who;
  if (!chunk.chunk) return "Compute " + std::string(pchunk_style_name(S.style)) + " does not use chunk/atom compute";
  if (!from_compute)
    return who + ": chunk/atom compute " + S.chunk + " is a bin style (fix ave/chunk reduces those); a chunk/atom compute over c_ID is taken";
  if (S.wants_id() && !compressed)
    return "compute property/chunk: id is not supported without compress yes in chunk/atom compute " + S.chunk +
           " (the chunk ID is the original ID there)";
  return std::string();
}

}  // namespace sf
