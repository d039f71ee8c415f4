// rlc_plan_host.cpp -- the plain C++ of csrc/rlc_plan.h (batch verification by random linear combination: the "keys repeat"
// test, the chunk-size rule, the bounds of what the device reports, the back-off of the key round) for
// tests/test_rlc_plan_host.py.  The header is plain C++, so this is the code the library runs.  A STAND-ALONE program: it reads
// commands from the file named on its command line and prints one line of results per command, so a host sanitizer build of it
// (-fsanitize=address,undefined) runs as it is.  TEST TOOL ONLY.
//   repeat   n u max_keys                                          -> rlc_keys_repeat
//   size     n u group auto lanes_per_round tri tri_max wide_max   -> rlc_chunk_size, then rlc_chunk_bound(n, that, u)
//   bound    items G u                                             -> rlc_chunk_bound
//   chunks   m n                                                   -> rlc_chunks_in_range
//   level    m u m_max items                                       -> rlc_level_in_range
//   list     mc m                                                  -> rlc_list_in_range
//   fallback m2 n                                                  -> rlc_fallback_in_range
//   backoff  ops                                                   -> one RlcBackoff driven by the letters of ops: P / F = a call
//            (take(enabled); where the round is taken it passes / fails), R = reset, E / D = the key round enabled / disabled;
//            per call "taken:skip:streak" as the call leaves them
// Numbers are decimal.
#include "../../bls-bn254_amd/csrc/rlc_plan.h"
#include <cstdio>
#include <fstream>
#include <string>

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <command file>\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::string cmd;
  while (in >> cmd) {
    if (cmd == "repeat") {
      size_t n, u, mx; in >> n >> u >> mx;
      std::printf("repeat %d\n", rlc_keys_repeat(n, u, mx) ? 1 : 0);
    } else if (cmd == "size") {
      size_t n, u, group, R, tri_max, wide; int is_auto, tri;
      in >> n >> u >> group >> is_auto >> R >> tri >> tri_max >> wide;
      const size_t G = rlc_chunk_size(n, u, group, is_auto != 0, R, tri != 0, tri_max, wide);
      std::printf("size %zu %zu\n", G, rlc_chunk_bound(n, G, u));
    } else if (cmd == "bound") {
      size_t items, G, u; in >> items >> G >> u;
      std::printf("bound %zu\n", rlc_chunk_bound(items, G, u));
    } else if (cmd == "chunks") {
      size_t m, n; in >> m >> n;
      std::printf("chunks %d\n", rlc_chunks_in_range(m, n) ? 1 : 0);
    } else if (cmd == "level") {
      size_t m, u, m_max, items; in >> m >> u >> m_max >> items;
      std::printf("level %d\n", rlc_level_in_range(m, u, m_max, items) ? 1 : 0);
    } else if (cmd == "list") {
      size_t mc, m; in >> mc >> m;
      std::printf("list %d\n", rlc_list_in_range(mc, m) ? 1 : 0);
    } else if (cmd == "fallback") {
      size_t m2, n; in >> m2 >> n;
      std::printf("fallback %d\n", rlc_fallback_in_range(m2, n) ? 1 : 0);
    } else if (cmd == "backoff") {
      std::string ops; in >> ops;
      RlcBackoff b;
      bool enabled = true;
      std::printf("backoff");
      for (char op : ops) {
        if (op == 'R') b.reset();
        else if (op == 'E' || op == 'D') enabled = op == 'E';
        else if (op == 'P' || op == 'F') {
          const bool taken = b.take(enabled);
          if (taken) { if (op == 'P') b.passed(); else b.failed(); }
          std::printf(" %d:%u:%u", taken ? 1 : 0, b.skip, b.streak);
        } else { std::fprintf(stderr, "unknown back-off letter %c\n", op); return 2; }
      }
      std::printf("\n");
    } else { std::fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    if (!in) { std::fprintf(stderr, "short command %s\n", cmd.c_str()); return 2; }
  }
  return 0;
}
