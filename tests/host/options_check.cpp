// Host-only checks of the table of tuning knobs and of the rule that resolves them (megahit_amd/csrc/mhx_options.h; no GPU, no libmhx).
// Prints "ok" and exits 0, or a message and exits 1.  With -DWRONG_FORM_PLAIN or -DWRONG_FORM_DERIVED it must not compile.
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>

#include "mhx_options.h"

using mhx::kNumOptions;
using mhx::kOptions;
using mhx::Opt;
using mhx::OptMap;
using mhx::OptScope;
using mhx::resolve_option;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "options_check:%d: %s\n", __LINE__, #cond);          \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

constexpr Opt kPlain = Opt::s1_stream_max, kDerived = Opt::s1_stream_max3;
static const char *const kPlainEnv = "MHX_S1_STREAM_MAX", *const kDerivedEnv = "MHX_S1_STREAM_MAX3";

static void the_table() {
  CHECK(kNumOptions > 50);
  std::set<std::string> names;
  size_t n_derived = 0;
  for (size_t i = 0; i < kNumOptions; ++i) {
    const mhx::OptInfo &o = kOptions[i];
    CHECK(o.name && *o.name && names.insert(o.name).second);
    std::string env = "MHX_";
    for (const char *p = o.name; *p; ++p) env += (char)toupper((unsigned char)*p);
    CHECK(env == o.env_name);
    n_derived += o.derived;
  }
  CHECK(n_derived == 5);
  CHECK(&mhx::opt_info(kPlain) == &kOptions[(size_t)kPlain]);
  CHECK(std::string(mhx::opt_info(kPlain).name) == "s1_stream_max" && std::string(mhx::opt_info(kPlain).env_name) == kPlainEnv);
  CHECK(mhx::opt_info(kPlain).dflt == 40000 && !mhx::opt_info(kPlain).derived);
  CHECK(std::string(mhx::opt_info(kDerived).name) == "s1_stream_max3" && std::string(mhx::opt_info(kDerived).env_name) == kDerivedEnv);
  CHECK(mhx::opt_info(kDerived).derived);
  // the one knob whose reads once disagreed: the documented default
  CHECK(mhx::opt_info(Opt::dist_sparse_marks).dflt == 0);
}

// explicit option, then a non-empty environment value (atoll), then the tuning file, then the default / the site's fallback
static void the_precedence() {
  unsetenv(kPlainEnv);
  unsetenv(kDerivedEnv);
  OptMap options, tuned;
  CHECK(resolve_option<kPlain>(options, tuned) == 40000);
  CHECK(resolve_option<kDerived>(options, tuned, 20000) == 20000 && resolve_option<kDerived>(options, tuned, 7) == 7);
  tuned["s1_stream_max"] = 30000;
  tuned["s1_stream_max3"] = 15000;
  CHECK(resolve_option<kPlain>(options, tuned) == 30000);
  CHECK(resolve_option<kDerived>(options, tuned, 20000) == 15000);  // (the fallback only when nothing else gives a value)
  setenv(kPlainEnv, "", 1);  // an empty value is no value
  setenv(kDerivedEnv, "", 1);
  CHECK(resolve_option<kPlain>(options, tuned) == 30000);
  CHECK(resolve_option<kDerived>(options, tuned, 20000) == 15000);
  tuned.clear();
  CHECK(resolve_option<kPlain>(options, tuned) == 40000);
  CHECK(resolve_option<kDerived>(options, tuned, 20000) == 20000);
  tuned["s1_stream_max"] = 30000;
  tuned["s1_stream_max3"] = 15000;
  setenv(kPlainEnv, "123", 1);
  setenv(kDerivedEnv, " -45x", 1);  // atoll: leading blanks, a sign, stops at the first other character
  CHECK(resolve_option<kPlain>(options, tuned) == 123);
  CHECK(resolve_option<kDerived>(options, tuned, 20000) == -45);
  setenv(kPlainEnv, "junk", 1);  // atoll of no number: 0, and still a value
  CHECK(resolve_option<kPlain>(options, tuned) == 0);
  options["s1_stream_max"] = 9;
  options["s1_stream_max3"] = 0;
  CHECK(resolve_option<kPlain>(options, tuned) == 9);
  CHECK(resolve_option<kDerived>(options, tuned, 20000) == 0);
  // by name (mhx_get_option): the same four steps, for a name of the table and for any other, with the caller's default
  CHECK(resolve_option(options, tuned, "s1_stream_max", 1) == 9);
  options.clear();
  setenv(kPlainEnv, "123", 1);
  CHECK(resolve_option(options, tuned, "s1_stream_max", 1) == 123);
  unsetenv(kPlainEnv);
  CHECK(resolve_option(options, tuned, "s1_stream_max", 1) == 30000);
  tuned.clear();
  CHECK(resolve_option(options, tuned, "s1_stream_max", 1) == 1 && resolve_option(options, tuned, "no_such_knob", 17) == 17);
  setenv("MHX_NO_SUCH_KNOB", "5", 1);
  CHECK(resolve_option(options, tuned, "no_such_knob", 17) == 5);
  unsetenv("MHX_NO_SUCH_KNOB");
  unsetenv(kDerivedEnv);
  // a typed set is an explicit option under the table's name
  mhx::set_option(options, Opt::dist_sparse_marks, 1);
  CHECK(options.size() == 1 && options.at("dist_sparse_marks") == 1 && resolve_option<Opt::dist_sparse_marks>(options, tuned) == 1);
}

static void the_scope() {
  unsetenv(kPlainEnv);
  unsetenv(kDerivedEnv);
  OptMap options, tuned;
  tuned["s1_stream_max"] = 30000;
  {  // nothing set: both put (a tuned default does not hold a put back), both gone afterwards
    OptScope s(options);
    s.put(kPlain, 5);
    s.put(kDerived, 6);
    CHECK(resolve_option<kPlain>(options, tuned) == 5 && resolve_option<kDerived>(options, tuned, 20000) == 6);
  }
  CHECK(options.empty() && resolve_option<kPlain>(options, tuned) == 30000);
  options["s1_stream_max"] = 9;       // an explicit option ...
  setenv(kDerivedEnv, "11", 1);       // ... and an environment value stay as they are
  options["sort_hybrid"] = 2;
  {
    OptScope s(options);
    s.put(kPlain, 5);
    s.put(kDerived, 6);
    s.put(Opt::s1_stream_sub_max, 0);
    CHECK(resolve_option<kPlain>(options, tuned) == 9 && resolve_option<kDerived>(options, tuned, 20000) == 11);
    CHECK(options.count("s1_stream_max3") == 0 && resolve_option<Opt::s1_stream_sub_max>(options, tuned) == 0);
  }
  CHECK(options.size() == 2 && options.at("s1_stream_max") == 9 && options.at("sort_hybrid") == 2);
  CHECK(resolve_option<Opt::s1_stream_sub_max>(options, tuned) == 1 && resolve_option<kDerived>(options, tuned, 20000) == 11);
  unsetenv(kDerivedEnv);
  options.clear();
  try {  // left by an exception: gone all the same
    OptScope s(options);
    s.put(kPlain, 5);
    throw 1;
  } catch (int) {
  }
  CHECK(options.empty());
}

int main() {
#ifdef WRONG_FORM_PLAIN
  OptMap o, t;
  return (int)resolve_option<kPlain>(o, t, 1);  // a knob with a default in the table takes no fallback
#endif
#ifdef WRONG_FORM_DERIVED
  OptMap o, t;
  return (int)resolve_option<kDerived>(o, t);  // a derived knob needs one
#endif
  the_table();
  the_precedence();
  the_scope();
  puts("ok");
  return 0;
}
