// Tuning knobs of the planner and the launchers: ONE process-wide table instead of ~70 environment variables.
//
// Rounds 1-5 read `getenv("SEFD_<KNOB>")` at 64 sites: a plan was a function of the environment at the moment it was built, and a stray variable
// changed what the library did.  Now every site reads this table through the typed reads below, and the table has exactly two writers:
//   * the single environment variable SEFD_TUNING="KNOB=value,KNOB=value,...", parsed ONCE, the first time the table is consulted; the parsed
//     pairs are kept, and they are what tune_clear() returns the table to;
//   * the C ABI: sefd_tuning_set(knob, value) (value NULL: unset) and sefd_tuning_clear() (include/sefd.h) - what the tests and the A/B tools call.
// A plan is therefore a function of its sefd_model_config and of this explicit table.  The knobs and their defaults: INTEGRATION.md section 6.
// No reader keeps a value: the planner reads a knob while it builds a plan, a launcher on every launch, the executor on every run.
#pragma once

namespace sefd {
bool tune_has(const char* knob);                        // set at all, whatever the value ("=0" included)
bool tune_on(const char* knob);                         // default on: false only when set to a text that atoi reads as 0
bool tune_is(const char* knob, int v);                  // opt in: true only when set and atoi(value) == v
long long tune_int(const char* knob, long long dflt);   // atoll(value) when set, else dflt; a caller with a valid range checks it itself
const char* tune_str(const char* knob);                 // sefd_tuning_get only.  nullptr when not set; valid until the knob is set again / cleared
void tune_set(const char* knob, const char* value);     // value nullptr: unset
void tune_clear();                                      // back to the pairs of SEFD_TUNING (an empty table when the variable is not set)
}  // namespace sefd
