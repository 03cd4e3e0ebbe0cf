// sf_env.h -- the one reader of the SF_* environment knobs (docs/knobs.md lists them).  Host only, no HIP headers.
// One function per idiom; numbers are parsed by atoi / atof ("abc" is 0, the empty string is "set, 0").  A function reads
// the environment when it is called: WHEN a knob is read -- in the engine's constructor, in the initialiser of a
// function-local static (first use, once per process) or on every use -- is decided where it is called, and the tests
// that switch knobs inside one process depend on it.
#pragma once
#include <cstdlib>

namespace sf {

// the value, or null when the variable is not set (paths, lists, words)
inline const char* env_str(const char* name) { return getenv(name); }
// presence only: "SF_X=0" and "SF_X=" count as set (the debug switches)
inline bool env_set(const char* name) { return getenv(name) != nullptr; }
inline int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
inline double env_double(const char* name, double dflt) { const char* v = getenv(name); return v ? atof(v) : dflt; }
// on / off: unset gives dflt, anything set is atoi(value) != 0
inline bool env_flag(const char* name, bool dflt) { const char* v = getenv(name); return v ? atoi(v) != 0 : dflt; }
// an override that has to know whether it was given: true and out = atoi(value) when set, out untouched when not
inline bool env_override(const char* name, int& out) { const char* v = getenv(name); if (v) out = atoi(v); return v != nullptr; }

}  // namespace sf
