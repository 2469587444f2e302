// The library's environment switches: the LIB / BOTH lines of switches.def as an enum and a table of (name, default), and the one
// function that reads the environment.  A site keeps its own `static const` around vt_switch(), so each is still read once, at
// first use.
#pragma once
#include <stdlib.h>

#define VT_SWITCH(name, rule, dflt, reader) VT_SWITCH_##reader(name, dflt)
#define VT_SWITCH_PY(name, dflt)
#define VT_SWITCH_BOTH(name, dflt) VT_SWITCH_LIB(name, dflt)

enum Switch {
#define VT_SWITCH_LIB(name, dflt) name,
#include "switches.def"
#undef VT_SWITCH_LIB
};
struct SwitchEntry { const char* name; const char* dflt; };
constexpr SwitchEntry SWITCH_TABLE[] = {
#define VT_SWITCH_LIB(name, dflt) {#name, dflt},
#include "switches.def"
#undef VT_SWITCH_LIB
};
#undef VT_SWITCH_BOTH
#undef VT_SWITCH_PY
#undef VT_SWITCH

// the variable's value as atol() reads it, the default's when it is unset
static inline long vt_switch(Switch s) {
  const char* e = getenv(SWITCH_TABLE[s].name);
  return atol(e ? e : SWITCH_TABLE[s].dflt);
}
