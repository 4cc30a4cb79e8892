// Prints one line per row of csrc/switches.h (tests/test_switches_host.py builds this from the header alone, with the host compiler):
//   <environment name> <option name or -> <kind> default=<v> 1=<v> 0=<v> [-5=<v> 100000=<v>]
// kind: + on when set, - off when set, i integer, s string; <v> after NAME=<value> is what read_switches() returns with the variable set
// to <value>; integer rows also list the two values that show their clamp.
#include "switches.h"
#include <cstdio>
#include <string>

using namespace sagen;

static std::string show(bool v) { return v ? "1" : "0"; }
static std::string show(long v) { return v == SW_UNSET ? "unset" : std::to_string(v); }
static std::string show(const char* v) { return v ? std::string("'") + v + "'" : "null"; }

int main() {
#define X(member, kind, dflt, env, opt, doc) unsetenv(env);
    SAGEN_SWITCHES(X)
#undef X
#define X(member, kind, dflt, env, opt, doc)                                                                  \
    {                                                                                                         \
        const char* option = opt;                                                                             \
        printf("%s %s %c default=%s", env, option ? option : "-", kind::tag, show(read_switches().member).c_str()); \
        for (const char* v : {"1", "0", "-5", "100000"}) {                                                    \
            if (kind::tag != 'i' && v[1]) continue;           /* the clamp values: integer rows only */       \
            setenv(env, v, 1);                                                                                \
            printf(" %s=%s", v, show(read_switches().member).c_str());                                        \
        }                                                                                                     \
        unsetenv(env);                                                                                        \
        printf("\n");                                                                                         \
    }
    SAGEN_SWITCHES(X)
#undef X
    return 0;
}
