// launch_forms_host.cpp -- the plain C++ of csrc/launch_forms.h (which device form runs at which size, and the settings'
// environment overrides) for tests/test_launch_forms_host.py.  The header is plain C++, so this is the code the library runs.  A
// STAND-ALONE program: it reads commands from the file named on its command line and prints one line of results per command, so a
// host sanitizer build of it (-fsanitize=address,undefined) runs as it is.  TEST TOOL ONLY.
// S stands for the eight settings: lanes_per_round wide wide_max tri_max tri_miller tri_fe split_easy quad_prep
//   defaults                       -> the eight settings of LaunchForms{}
//   env      cus k name value ...  -> the eight settings of forms_from_env over the k variables given (values without blanks)
//   fe_hard  S n                   -> fe_hard_form: wide / tri / lane
//   fe_split S n                   -> fe_easy_split
//   miller   S n                   -> miller_form
//   table    S n mask              -> table_miller_form
//   two      S n mask chunk        -> raw_two_per_lane
//   prep     S u                   -> prepare_on_quads
//   small    S n per_tuple_fe      -> small_for_prepared
//   grouped  S n                   -> grouped_whatever_keys
// Numbers are decimal.
#include "../../bls-bn254_amd/csrc/launch_forms.h"
#include <cstdio>
#include <fstream>
#include <map>
#include <string>

static std::map<std::string, std::string> g_env;
static const char* env_get(const char* name) {
  const auto it = g_env.find(name);
  return it == g_env.end() ? nullptr : it->second.c_str();
}
static const char* name_of(Form f) { return f == Form::WIDE ? "wide" : f == Form::TRI ? "tri" : "lane"; }
static void print_settings(const char* cmd, const LaunchForms& F) {
  std::printf("%s %zu %d %zu %zu %d %d %d %d\n", cmd, F.lanes_per_round, F.wide ? 1 : 0, F.wide_max, F.tri_max, F.tri_miller ? 1 : 0, F.tri_fe ? 1 : 0,
              F.split_easy ? 1 : 0, F.quad_prep ? 1 : 0);
}
static LaunchForms read_settings(std::istream& in) {
  LaunchForms F;
  int wide, tm, tf, se, qp;
  in >> F.lanes_per_round >> wide >> F.wide_max >> F.tri_max >> tm >> tf >> se >> qp;
  F.wide = wide != 0; F.tri_miller = tm != 0; F.tri_fe = tf != 0; F.split_easy = se != 0; F.quad_prep = qp != 0;
  return F;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <command file>\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::string cmd;
  while (in >> cmd) {
    if (cmd == "defaults") {
      print_settings("defaults", LaunchForms{});
    } else if (cmd == "env") {
      int cus; size_t k; in >> cus >> k;
      g_env.clear();
      for (size_t i = 0; i < k; ++i) { std::string name, value; in >> name >> value; g_env[name] = value; }
      print_settings("env", forms_from_env(env_get, cus));
    } else {
      const LaunchForms F = read_settings(in);
      size_t n; in >> n;
      if (cmd == "fe_hard") std::printf("fe_hard %s\n", name_of(fe_hard_form(F, n)));
      else if (cmd == "fe_split") std::printf("fe_split %d\n", fe_easy_split(F, n) ? 1 : 0);
      else if (cmd == "miller") std::printf("miller %s\n", name_of(miller_form(F, n)));
      else if (cmd == "table") { unsigned mask; in >> mask; std::printf("table %s\n", name_of(table_miller_form(F, n, mask))); }
      else if (cmd == "two") { unsigned mask; size_t chunk; in >> mask >> chunk; std::printf("two %d\n", raw_two_per_lane(F, n, mask, chunk) ? 1 : 0); }
      else if (cmd == "prep") std::printf("prep %d\n", prepare_on_quads(F, n) ? 1 : 0);
      else if (cmd == "small") { int fe; in >> fe; std::printf("small %d\n", small_for_prepared(F, n, fe != 0) ? 1 : 0); }
      else if (cmd == "grouped") std::printf("grouped %d\n", grouped_whatever_keys(F, n) ? 1 : 0);
      else { std::fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    if (!in) { std::fprintf(stderr, "short command %s\n", cmd.c_str()); return 2; }
  }
  return 0;
}
