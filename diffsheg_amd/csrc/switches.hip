// C ABI over the table of runtime switches (switches.h): host code only, no kernel and no GPU call.
#include "switches.h"

#include <cstring>

#include "../../include/diffsheg_hip.h"
#include "dsh_common.h"

extern "C" {
int32_t dsh_switch_count(void) { return dsh::SW_COUNT; }

int dsh_switch_info(int32_t i, const char** name, const char** default_text, int32_t* when, int32_t* cls, const char** help) {
    DSH_REQUIRE(i >= 0 && i < dsh::SW_COUNT, "dsh_switch_info: no such entry");
    const dsh::SwitchInfo& e = dsh::kSwitches[i];
    if (name) *name = e.name;
    if (default_text) *default_text = e.def;
    if (when) *when = e.when;
    if (cls) *cls = e.cls;
    if (help) *help = e.help;
    return e.kind;
}

int dsh_switch_read(const char* name, int32_t* is_set, int64_t* value) {
    DSH_REQUIRE(name, "dsh_switch_read: null name");
    for (int i = 0; i < dsh::SW_COUNT; ++i) {
        if (strcmp(name, dsh::kSwitches[i].name) != 0) continue;
        const dsh::SwitchValue v = dsh::switch_value((dsh::Switch)i);      // latched for a PROCESS entry, fresh otherwise — as the library reads it
        if (is_set) *is_set = v.set;
        if (value) *value = v.set ? v.v : dsh::kSwitches[i].def_int;
        return 0;
    }
    for (const dsh::SwitchDerived& d : dsh::kSwitchDerived) {
        if (strcmp(name, d.name) != 0) continue;
        if (is_set) *is_set = 0;
        if (value) *value = d.fn();
        return 0;
    }
    DSH_REQUIRE(false, "dsh_switch_read: not a switch of the table nor a derivation");
    return -1;
}

}  // extern "C"
