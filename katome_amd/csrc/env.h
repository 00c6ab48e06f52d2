// env.h -- the environment switches (KATOME_*) read one way.  Host only, nothing of HIP.  A switch that is to be read once per process
// is kept in a function-local static by its reader; one that is to be read on every call is asked for on every call.
#pragma once
#include <stdlib.h>
#include <string.h>

namespace katome {

static inline bool env_is(const char* name, const char* value) { const char* e = getenv(name); return e && !strcmp(e, value); }
// the switch as a number (atoi); `unset` when it is not in the environment
static inline int env_int(const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; }
// unset = true: on unless it says 0; unset = false: off unless it says a number other than 0
static inline bool env_flag(const char* name, bool unset) { return env_int(name, unset ? 1 : 0) != 0; }

}  // namespace katome
