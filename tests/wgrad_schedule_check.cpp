// Host check of the weight-gradient schedule (ssak_amd/csrc/wgrad_schedule.h) with recording callables: no GPU, no HIP.
// Built with -fsanitize=address,undefined and run by tests/test_wgrad_schedule.py; exit status 0 = every case held.
#include "../ssak_amd/csrc/wgrad_schedule.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      std::fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);                   \
      std::fprintf(stderr, "\n");                          \
      std::exit(1);                                        \
    }                                                      \
  } while (0)

namespace {

struct Product {
  int tiles, set;
};
struct Range {
  long off, cnt, last;      // last: sequence number of the product the range waits for, -1: none
  long launched_when = -1;  // products launched when it was announced
};
using Partition = std::vector<std::vector<int>>;  // product sequence numbers per launch

constexpr int CAP = 48, ROUND = 256;

// The rule, written independently of the header: walk the products in push order; a layer that begins closes the open launch
// if that still holds a product of the layer's set; a product closes it if it would pass 256 tiles or 48 products.
Partition model(const std::vector<Product>& prod, const std::vector<int>& layer_begin /* per product: set of a layer beginning here, else -1 */) {
  Partition out;
  std::vector<int> cur;
  int tiles = 0;
  auto close = [&] { if (!cur.empty()) out.push_back(cur); cur.clear(); tiles = 0; };
  for (int i = 0; i < (int)prod.size(); ++i) {
    bool reads_set = false;
    for (int j : cur) reads_set |= layer_begin[i] >= 0 && prod[j].set == layer_begin[i];
    if (reads_set) close();
    if (!cur.empty() && (tiles + prod[i].tiles > ROUND || (int)cur.size() == CAP)) close();
    cur.push_back(i);
    tiles += prod[i].tiles;
  }
  close();
  return out;
}

struct Result {
  Partition launches;
  std::vector<int> launch_tiles;
};

// Drives the schedule the way the backward does: the head's product and range, then layers L-1 .. 0, then the final flush.
Result run(int L, bool head, const int layer_tiles[4], int head_tiles, const std::vector<bool>& keep, const char* what) {
  std::vector<Product> prod;        // every product pushed, by sequence number
  std::vector<int> layer_begin;     // see model()
  std::vector<int> unlaunched;      // sequence numbers still queued
  int slot_seq[CAP];                // what the caller keeps by slot
  long launched = 0;
  Result res;
  std::vector<Range> expected, announced;

  auto launch = [&](int n, int tiles) -> int {
    CHECK(n >= 1 && n <= CAP, "%s: launch of %d products", what, n);
    CHECK(n == 1 || tiles <= ROUND, "%s: %d products with %d tiles in one launch", what, n, tiles);
    CHECK(n == (int)unlaunched.size(), "%s: launch of %d products, %zu queued", what, n, unlaunched.size());
    int sum = 0;
    for (int i = 0; i < n; ++i) {
      CHECK(slot_seq[i] == unlaunched[i], "%s: slot %d holds product %d, expected %d", what, i, slot_seq[i], unlaunched[i]);
      sum += prod[slot_seq[i]].tiles;
    }
    CHECK(sum == tiles, "%s: launch reports %d tiles, its products have %d", what, tiles, sum);
    res.launches.push_back(unlaunched);
    res.launch_tiles.push_back(tiles);
    launched += n;
    unlaunched.clear();
    return 0;
  };
  auto announce = [&](long off, long cnt) { announced.push_back(Range{off, cnt, 0, launched}); };
  WgradSchedule<decltype(launch)&, decltype(announce)&> s(launch, announce);
  using S = decltype(s);

  auto pending_ok = [&] {
    CHECK(s.pending_ranges() <= S::MAX_RANGES && s.pending_ranges() == (int)(expected.size() - announced.size()),
          "%s: %d ranges pending, %zu expected", what, s.pending_ranges(), expected.size() - announced.size());
  };
  auto push = [&](int tiles, int set, int begins_layer_of_set) {
    int slot = -1;
    CHECK(s.push(tiles, set, &slot) == 0, "%s: push failed", what);
    CHECK(slot == (int)unlaunched.size() && slot < CAP, "%s: slot %d with %zu queued", what, slot, unlaunched.size());
    slot_seq[slot] = (int)prod.size();
    unlaunched.push_back((int)prod.size());
    prod.push_back(Product{tiles, set});
    layer_begin.push_back(begins_layer_of_set);
    CHECK(s.queued() == (int)unlaunched.size(), "%s: queued() = %d", what, s.queued());
  };
  auto range = [&](long off, long cnt, bool waits) {
    expected.push_back(Range{off, cnt, waits ? (long)prod.size() - 1 : -1});
    CHECK((waits ? s.announce_after_last_product(off, cnt) : s.announce_in_order(off, cnt)) == 0, "%s: range refused", what);
    pending_ok();
  };

  if (head) {
    push(head_tiles, -1, -1);
    range(7, 3, true);
  }
  int kept = 0;
  for (int l = L - 1; l >= 0; --l) {
    const long off = 1000 + 100L * l, cnt = 50 + l;
    if (!keep[l]) {
      range(off, cnt, false);
      continue;
    }
    const int set = kept++ % WGRAD_SETS;
    CHECK(s.reserve_set(set) == 0, "%s: reserve_set failed", what);
    for (int i : unlaunched) CHECK(prod[i].set != set, "%s: layer %d starts on set %d while product %d still reads it", what, l, set, i);
    CHECK(!s.uses_set(set), "%s: uses_set(%d) after reserve_set", what, set);
    for (int i = 0; i < 4; ++i) push(layer_tiles[i], set, i == 0 ? set : -1);
    range(off, cnt, true);
  }
  CHECK(s.flush() == 0, "%s: final flush failed", what);
  CHECK(s.queued() == 0 && s.queued_tiles() == 0 && s.pending_ranges() == 0 && unlaunched.empty(), "%s: something left after the final flush", what);

  // the announced sequence is exactly [head], L-1 .. 0, each once, and none before the launch holding its last product
  CHECK(announced.size() == expected.size() && (int)expected.size() == L + (head ? 1 : 0), "%s: %zu ranges announced, %zu expected",
        what, announced.size(), expected.size());
  for (size_t i = 0; i < expected.size(); ++i) {
    CHECK(announced[i].off == expected[i].off && announced[i].cnt == expected[i].cnt, "%s: announcement %zu is (%ld, %ld), expected (%ld, %ld)",
          what, i, announced[i].off, announced[i].cnt, expected[i].off, expected[i].cnt);
    CHECK(announced[i].launched_when > expected[i].last, "%s: range %zu announced before product %ld was launched", what, i, expected[i].last);
  }
  const Partition want = model(prod, layer_begin);
  CHECK(res.launches == want, "%s: the launches differ from the model's partition (%zu vs %zu launches)", what, res.launches.size(), want.size());
  return res;
}

unsigned rng_state;
double uniform() {  // (an LCG of our own: the same patterns with every compiler and library)
  rng_state = rng_state * 1664525u + 1013904223u;
  return (rng_state >> 8) / 16777216.0;
}

}  // namespace

int main() {
  const int layer_counts[] = {1, 2, 12, 24, 48, SSAK_MAX_LAYERS};
  const int tiles[3][4] = {{1, 1, 1, 1}, {36, 36, 9, 27}, {64, 64, 16, 48}};  // push order w2, w1, wo, wqkv
  const int head_tiles[3] = {1, 3, 4};
  static_assert(SSAK_MAX_LAYERS == 64, "the issue's largest case");
  long cases = 0;
  for (int L : layer_counts)
    for (int head = 0; head < 2; ++head)
      for (int t = 0; t < 3; ++t) {
        std::vector<std::vector<bool>> patterns;
        patterns.push_back(std::vector<bool>(L, true));
        patterns.push_back(std::vector<bool>(L, false));
        std::vector<bool> alt(L), last(L, false), first(L, false);
        for (int l = 0; l < L; ++l) alt[l] = l % 2 == 0;
        last[L - 1] = true;  // only layer L-1 kept: every other range queues behind it and the head
        first[0] = true;
        patterns.push_back(alt);
        patterns.push_back(last);
        patterns.push_back(first);
        for (double prob : {0.9, 0.5})
          for (unsigned seed = 0; seed < 200; ++seed) {
            rng_state = seed * 2654435761u + (unsigned)(prob * 1000) + 97u * L;
            std::vector<bool> k(L);
            for (int l = 0; l < L; ++l) k[l] = uniform() < prob;
            patterns.push_back(k);
          }
        for (size_t i = 0; i < patterns.size(); ++i) {
          char what[96];
          std::snprintf(what, sizeof what, "L=%d head=%d tiles=%d pattern=%zu", L, head, t, i);
          run(L, head != 0, tiles[t], head_tiles[t], patterns[i], what);
          ++cases;
        }
      }
  {
    // base tiles, a head, 12 layers all kept: 3 + 108 + 108 + 36 = 255 tiles in 1 + 4 + 4 + 1 = 10 products (layer 9's next,
    // 36 tiles, would make 291), then layer 9's remaining 72 + 108 + 36 + 36 = 252 tiles in 3 + 4 + 2 = 9 products (the next,
    // 9 tiles, would make 261)
    const Result r = run(12, true, tiles[1], 3, std::vector<bool>(12, true), "base 12 layers");
    CHECK(r.launches.size() >= 2 && r.launches[0].size() == 10 && r.launch_tiles[0] == 255 && r.launches[1].size() == 9 && r.launch_tiles[1] == 252,
          "base: first launches are %zu / %d and %zu / %d", r.launches[0].size(), r.launch_tiles[0], r.launches[1].size(), r.launch_tiles[1]);
  }
  {
    // a product alone is never refused, and the FIFO refuses the entry past its capacity instead of writing it
    int launches = 0, ranges = 0, slot = -1;
    auto launch = [&](int, int) { ++launches; return 0; };
    auto announce = [&](long, long) { ++ranges; };
    WgradSchedule<decltype(launch)&, decltype(announce)&> s(launch, announce);
    using S = decltype(s);
    CHECK(s.push(100000, 0, &slot) == 0 && slot == 0 && launches == 0, "a large product alone");
    CHECK(s.push(1, 1, &slot) == 0 && slot == 0 && launches == 1, "the product after it starts the next launch");
    for (int i = 0; i < S::MAX_RANGES; ++i) CHECK(s.announce_after_last_product(i, 1) == 0, "range %d refused", i);
    CHECK(s.pending_ranges() == S::MAX_RANGES && ranges == 0, "%d pending", s.pending_ranges());
    CHECK(s.announce_in_order(99, 1) == S::ERR_RANGES && s.announce_after_last_product(99, 1) == S::ERR_RANGES, "an append past the capacity");
    CHECK(s.flush() == 0 && ranges == S::MAX_RANGES && s.pending_ranges() == 0, "%d ranges after the flush", ranges);
  }
  std::printf("wgrad schedule: %ld cases ok\n", cases + 2);
  return 0;
}
