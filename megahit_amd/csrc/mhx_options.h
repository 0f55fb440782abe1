// Every tuning knob of libmhx, declared once: its name and its default.  The host code reads a knob as c->opt<Opt::name>() and
// nowhere repeats the name as a string or the default as a number; include/mhx.h and INTEGRATION.md say what each knob does
// (tests/test_knobs_documented.py holds them to this table).  Plain C++: no HIP, no other header of the library
// (tests/host/options_check.cpp drives it on the CPU).
//
// A value is resolved in four steps: the explicit option (mhx_set_option), else a non-empty MHX_<NAME> in the environment (atoll),
// else the installation's mhx_tuning.conf, else the default.  A *derived* knob has no default a table could hold — it follows a
// size only the reading site knows — and is read as c->opt<Opt::name>(fallback); using the wrong form for a knob does not compile.
//
// A new knob: one line below, in the group of the file that owns it, a description in include/mhx.h, and reads through Opt::name.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

// X(name, default) | D(name): derived, the default comes from the reading site
#define MHX_OPTIONS(X, D)          \
  /* capi.hip */                   \
  X(edges_reserve_permille, 1000)  \
  X(fetch_pinned, 1)               \
  X(dist_marks_one_pass, 1)        \
  /* sort.hip */                   \
  X(sort_unit_runs, 1)             \
  X(sort_xcd_units, 1)             \
  X(sort_loaded_ut2, 0)            \
  X(sort_rank_uniform, 1)          \
  X(sort_hybrid, 1)                \
  X(sort_hybrid_min, 1 << 16)      \
  X(sort_hybrid_margin_ps, 6)      \
  X(sort_hybrid_bits, 0)           \
  /* iterate.hip */                \
  X(iterate_prefix_filter, 1)      \
  /* sdbg_tips.hip */              \
  X(tips_candidate_list, 1)        \
  /* sdbg_index.hip */             \
  D(sdbg_hist_flush_tiles)         \
  /* kmsort_emu.hip */             \
  X(kmsort_emu_legacy, 0)          \
  /* passes.hip */                 \
  X(s2_filter_in_extract, 1)       \
  /* comm.hip */                   \
  X(dist_presort, 1)               \
  X(dist_max_items, 0)             \
  X(count_skm_dist, 0)             \
  /* count.hip */                  \
  X(count_seg, 1)                  \
  X(count_seg_bits, 0)             \
  X(count_extract_fixed, 1)        \
  X(count_seg_la, 3)               \
  /* s1.hip */                     \
  X(s1_seg_bits, 0)                \
  X(s1_seg, 1)                     \
  X(s1_stream, 1)                  \
  X(s1_stream_wide, 1)             \
  X(s1_stream_max, 40000)          \
  X(s1_stream_sub_max, 1)          \
  D(s1_stream_max3)                \
  X(s1_stream_bits, 0)             \
  X(s1_stream_sub0, -1)            \
  X(s1_pos_bits, 0)                \
  X(dist_sparse_marks, 0)          \
  X(s1_seg_per, 8)                 \
  X(s1_seg_la, 3)                  \
  X(s1_stream_direct, 1)           \
  X(s1_stream_probes, 1024)        \
  D(s1_stream_fill)                \
  X(s1_giant, 1)                   \
  X(s1_giant_min, 262144)          \
  X(s1_pack_fixed, 1)              \
  X(s1_agg_wide, 0)                \
  X(count_stream, 1)               \
  X(count_event_share, 4)          \
  X(count_giant, 1)                \
  /* s1_front.hip */               \
  X(s1_bucket_hist_fast, 1)        \
  X(s1_digit_hist_roll, 1)         \
  X(count_stream_wide, 1)          \
  X(s1_var_fast, 1)                \
  X(s1_var_min_fill, 50)           \
  X(s1_extract_fast, 1)            \
  X(s1_filter_in_gen, 1)           \
  X(s1_fused_first_pass, 1)        \
  X(s1_digit_hist_blocked, 1)      \
  X(s1_digit_hist_plain, 1)        \
  X(s1_gen_any_order, 1)           \
  X(s1_gen_blocked, 0)             \
  X(s1_gen_roll, 1)                \
  X(s1_extract_items, 4)           \
  X(s1_digit_hist_preload, 0)      \
  /* s1_tile.hip */                \
  X(s1_mercy_regions, 1)           \
  /* s1_skm.hip */                 \
  X(s1_skm, 1)                     \
  X(s1_skm_min_windows, 1 << 22)   \
  X(s1_skm_bin_bits, 0)            \
  X(count_skm, 1)                  \
  X(s1_skm_max_m, 2)               \
  X(dist_skm, 1)                   \
  X(s1_skm_passes, 0)              \
  X(s1_skm_cap_pct, 36)            \
  X(s1_skm_pass_gb, 48)            \
  X(s1_skm_split, 1)               \
  D(s1_skm_split_stage)            \
  X(s1_skm_make_grid, 0)           \
  X(s1_skm_hp, 1)                  \
  X(s1_skm_rep, 0)                 \
  X(s1_skm_rep_slots, 64)          \
  X(s1_skm_giant, 0)               \
  X(s1_skm_giant_max, 1 << 21)     \
  X(s1_skm_giant_keys, 4096)       \
  X(s1_skm_giant_work_pct, 25)     \
  X(s1_skm_giant_slices, 0)        \
  X(s1_skm_max_bin, 1 << 16)       \
  X(s1_skm_tags, 0)                \
  X(s1_skm_deal, 2)                \
  X(count_skm_group, 2)            \
  X(count_skm_ev_cap, 0)           \
  /* s2.hip */                     \
  X(sdbg_fast, 1)                  \
  D(sdbg_fast_halo)                \
  X(sdbg_fast_tile, 2048)          \
  X(sdbg_fast_keep, 1)             \
  X(sdbg_fast_keep_max_mb, 4096)   \
  X(s2_bound_from_s1, 1)           \
  X(s2_dummy_list, 1)              \
  X(s2_dummy_list_cap, 0)          \
  X(s2_agg_from_count, 1)          \
  X(s2_count_budget_mb, 0)         \
  X(s2_count_pass_items, 0)        \
  X(s2_pre_hist, 1)                \
  X(s2_agg_in_place, 1)

namespace mhx {

#define MHX_OPT_PLAIN(name, dflt) name,
#define MHX_OPT_DERIVED(name) name,
enum class Opt : int { MHX_OPTIONS(MHX_OPT_PLAIN, MHX_OPT_DERIVED) };
#undef MHX_OPT_PLAIN
#undef MHX_OPT_DERIVED

struct OptInfo {
  const char *name;
  char env_name[48];
  long long dflt;  // (derived: unused)
  bool derived;
};

// the environment's name for a knob: MHX_ and the name in upper case; out holds cap bytes, the end included
constexpr void opt_env_name(const char *name, char *out, size_t cap) {
  const char pre[] = "MHX_";
  size_t n = 0;
  for (const char *p = pre; *p && n + 1 < cap; ++p) out[n++] = *p;
  for (const char *p = name; *p && n + 1 < cap; ++p) out[n++] = *p >= 'a' && *p <= 'z' ? (char)(*p - 'a' + 'A') : *p;
  out[n] = 0;
}
constexpr OptInfo make_opt_info(const char *name, long long dflt, bool derived) {
  OptInfo o{name, {}, dflt, derived};
  opt_env_name(name, o.env_name, sizeof o.env_name);
  return o;
}

#define MHX_OPT_PLAIN(name, dflt) make_opt_info(#name, dflt, false),
#define MHX_OPT_DERIVED(name) make_opt_info(#name, 0, true),
inline constexpr OptInfo kOptions[] = {MHX_OPTIONS(MHX_OPT_PLAIN, MHX_OPT_DERIVED)};
#undef MHX_OPT_PLAIN
#undef MHX_OPT_DERIVED
inline constexpr size_t kNumOptions = sizeof kOptions / sizeof kOptions[0];
constexpr const OptInfo &opt_info(Opt o) { return kOptions[(size_t)o]; }

using OptMap = std::map<std::string, long long>;

// the four steps, over the handle's two maps
inline long long resolve_option(const OptMap &options, const OptMap &tuned, const char *name, const char *env_name, long long dflt) {
  auto it = options.find(name);
  if (it != options.end()) return it->second;
  const char *e = getenv(env_name);
  if (e && *e) return atoll(e);
  auto tu = tuned.find(name);
  return tu != tuned.end() ? tu->second : dflt;
}
// ... for a name and a default the caller brings (mhx_get_option: any name, in the table or not)
inline long long resolve_option(const OptMap &options, const OptMap &tuned, const char *name, long long dflt) {
  std::string env(strlen(name) + 5, '\0');
  opt_env_name(name, &env[0], env.size());
  return resolve_option(options, tuned, name, env.c_str(), dflt);
}
// ... for a knob of the table (mhx_ctx::opt<O>() and opt<O>(fallback) are these two)
template <Opt O>
long long resolve_option(const OptMap &options, const OptMap &tuned) {
  static_assert(!opt_info(O).derived, "a derived knob has no default of its own: read it as opt<Opt::name>(fallback)");
  return resolve_option(options, tuned, opt_info(O).name, opt_info(O).env_name, opt_info(O).dflt);
}
template <Opt O>
long long resolve_option(const OptMap &options, const OptMap &tuned, long long fallback) {
  static_assert(opt_info(O).derived, "this knob has its default in the table: read it as opt<Opt::name>()");
  return resolve_option(options, tuned, opt_info(O).name, opt_info(O).env_name, fallback);
}

inline void set_option(OptMap &options, Opt o, long long v) { options[opt_info(o).name] = v; }

// Knobs a code path sets for what it calls unless the caller set them: put() leaves a knob alone that an explicit option or the
// environment already gives, and what it did put is gone again when the scope is left, however.
class OptScope {
 public:
  explicit OptScope(OptMap &options) : options_(options) {}
  OptScope(const OptScope &) = delete;
  OptScope &operator=(const OptScope &) = delete;
  void put(Opt o, long long v) {
    if (options_.count(opt_info(o).name) || getenv(opt_info(o).env_name)) return;
    options_[opt_info(o).name] = v;
    put_.push_back(o);
  }
  ~OptScope() {
    for (Opt o : put_) options_.erase(opt_info(o).name);
  }

 private:
  OptMap &options_;
  std::vector<Opt> put_;
};

}  // namespace mhx
