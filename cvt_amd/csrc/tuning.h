// tuning.h -- the values cvtmi_set_tuning sets.  tuning.def lists them, one line per key: name, default, rule, flags.  Each line
// becomes one object `tune_<name>` (defined in api.hip, where the compiler is told to refuse anything but constant initialisation), which the dispatch and planner code reads on the
// host with get() / geti(); tune_all[] holds them in the order of the list, for cvtmi_set_tuning / cvtmi_get_tuning to walk.
#pragma once
#include <stdint.h>

#include <atomic>

namespace cvtmi {

enum TuneFlag { REPLAN = 1, ENV_DEFAULT = 2 };   // a set rebuilds the cached adc_scan16h item tables; default from the environment

struct Tunable {
    enum Rule { kReject, kClamp, kBool, kHook };   // outside lo .. hi: refused / moved to the nearer bound; v != 0; hook decides
    // a key whose rule is none of the above: normalises *v, or refuses it with the status it returns (and its own message)
    typedef int (*Hook)(int64_t *v);

    const char *const name;
    const int64_t def;
    const Rule rule;
    const int64_t lo, hi;
    const Hook hook;
    const int flags;
    std::atomic<int64_t> v;

    constexpr Tunable(const char *name_, int64_t def_, Rule rule_, int64_t lo_, int64_t hi_, Hook hook_, int flags_)
        : name(name_), def(def_), rule(rule_), lo(lo_), hi(hi_), hook(hook_), flags(flags_), v(def_) {}
    int64_t get() const { return v.load(std::memory_order_relaxed); }
    int geti() const { return (int)get(); }
};

#define TUNE(name, def, rule, flags) extern Tunable tune_##name;
#include "tuning.def"
#undef TUNE
extern Tunable *const tune_all[];

}  // namespace cvtmi
