// The reader of the switch table (fg_switches.h): environment -> handle members, handle members -> JSON.
#include <cstdlib>
#include "fg_mb.h"

int fg_switch_parse(const char* text, FgSwitchRule rule, int def) {
    if (rule == FG_SW_SET) return text != nullptr;
    if (!text) return def;
    const int v = atoi(text);
    switch (rule) {
        case FG_SW_POS: return v > 0 ? v : def;
        case FG_SW_ON: case FG_SW_OFF: case FG_SW_TRI: return v != 0;
        case FG_SW_ONE: return v == 1;
        case FG_SW_ALL: return v == 1 ? def : v;
        default: return v;
    }
}

namespace {
template <class S> struct Switch { const char* var; int def; FgSwitchRule rule; int& (*at)(S&); };
#define FG_SW_ROW(var, member, def, rule, scope, results, what) {#var, def, FG_SW_##rule, [](auto& s) -> int& { return s.member; }},
#define FG_SW_GLOBAL(var, global, def, rule, scope, results, what) {#var, def, FG_SW_##rule, [](auto&) -> int& { return global; }},
const Switch<fg_state> kSingle[] = {FG_COMMON_SWITCHES(FG_SW_ROW) FG_SB_SWITCHES(FG_SW_ROW) FG_PROCESS_SWITCHES(FG_SW_GLOBAL)};
const Switch<fg_mb_state> kMulti[] = {FG_COMMON_SWITCHES(FG_SW_ROW) FG_MB_SWITCHES(FG_SW_ROW) FG_PROCESS_SWITCHES(FG_SW_GLOBAL)};

template <class S, size_t N> void read(S* s, const Switch<S> (&table)[N]) {
    for (const Switch<S>& w : table) {
        int& member = w.at(*s);
        if (&member == &fg_htrace_on || &member == &fg_roctx_on) continue;      // (process scope: read where the library is loaded)
        const char* text = getenv(w.var);
        member = fg_switch_parse(text, w.rule, w.def);
        if (&member == &s->adv_jacobi) s->adv_jacobi_env = text != nullptr;
    }
    if (FG_F64 || !s->poll.spin) s->poll.words = 0;      // (no result words there: fg_poll_create)
}
template <class S, size_t N> void json(const S* s, const Switch<S> (&table)[N], std::string& out) {
    for (const Switch<S>& w : table) fg_json_put(out, w.var, w.at(*const_cast<S*>(s)));
}
}  // namespace

void fg_switches_read(fg_state* s) { read(s, kSingle); }
void fg_switches_read(fg_mb_state* s) {
    read(s, kMulti);
#if FG_MB_F64
    // the fp64 build runs the one-cell-per-thread kernels: the four-cell forms are well-formed in doubles but neither measured nor
    // tested there, the on-chip / cluster CG are written for 32-bit words (fg_mb.h)
    s->dbg_vec_mask = 0; s->onchip_mode = 0; s->dbg_oc_agg = 0; s->cl_mode = 0;
#endif
}
void fg_switches_json(const fg_state* s, std::string& out) { json(s, kSingle, out); }
void fg_switches_json(const fg_mb_state* s, std::string& out) { json(s, kMulti, out); }

void fg_json_put(std::string& out, const char* key, long long value) { out += std::string(out.back() == '{' ? "\"" : ", \"") + key + "\": " + std::to_string(value); }
int fg_json_out(const std::string& out, char* buf, int n) {
    if ((int)out.size() < n) memcpy(buf, out.c_str(), out.size() + 1);
    return (int)out.size() < n ? FG_OK : (int)out.size() + 1;
}

extern "C" int fg_switch_values(int32_t family, char* buf, int32_t n) {
    FG_REQUIRE((family == 0 || family == 1) && buf && n > 0, FG_ERR_INVALID_ARG, "fg_switch_values: bad argument");
    std::string out = "{";
    const auto values = [&](auto s) { fg_switches_read(&s); fg_switches_json(&s, out); };      // (a handle's worth of members, no device)
    family == 0 ? values(fg_state{}) : values(fg_mb_state{});
    return fg_json_out(out + "}", buf, n);
}
