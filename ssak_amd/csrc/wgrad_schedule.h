// Schedule of the backward's weight-gradient products and of the gradient ranges it announces (w2v2_engine.hip).
//
// Weight-gradient products are not on the critical path of the backward: they are queued and launched together as ONE grouped
// GEMM instead of four launches per layer that each need split-K slabs and a reduction pass.  Under data parallelism a finished
// gradient range is announced for the bucketed all-reduce.  This header is the POLICY alone: per product it needs the tile count
// and the buffer set, and it launches and announces through two callables.  Host code without HIP or engine types, so that
// tests/wgrad_schedule_check.cpp drives it under the address and undefined-behaviour sanitizers without a GPU.  The caller
// keeps the products' descriptors in arrays of CAP entries indexed by the slot push() hands out, and decides HOW a batch is
// launched (the engine: fp32 one by one, >= 160 tiles grouped, else split-K one by one).
//
// Invariants:
//   * Greedy packing.  Launches hold at most one round of 256 x 256 tiles (a base layer has 108: pairs of layers filled 216 of
//     256 workgroups and LayerDrop left an odd layer over in half of the steps, which then ran as four split-K launches): a
//     product that would take the queue past ROUND_TILES tiles or past CAP products first flushes what is queued, so launches
//     hold ~2.4 base layers and a layer's products may go out in two launches.  A product alone is never refused, whatever its
//     size.  (All kept layers in one multi-round launch was measured slower on one GPU: see make_plan.)
//   * Buffer sets.  The operands of a layer's products live in set (kept layers so far) % WGRAD_SETS.  reserve_set(s), called
//     before a layer starts writing set s, launches what is queued if any of it still reads set s.  Three sets: a layer's last
//     product may wait for the launch after next.
//   * Announcements are ONE FIFO in layer order: the lm_head range first when there is one, then layers L-1 down to 0.  A
//     data-parallel caller pairs the k-th announcement of every rank in one collective and LayerDrop decisions differ between
//     ranks, so a dropped layer's (zero) range must never overtake the kept layers still waiting: ranks would pair different
//     ranges and the trainer deadlocks.  A range whose products are pending is announced right after the launch that contains
//     its last product; a range with nothing to wait for is announced at once only if nothing is pending ahead of it, and
//     otherwise queues behind what is.  Every range is announced exactly once, by the last flush() at the latest.
//   * Bounded.  The FIFO holds MAX_RANGES = SSAK_MAX_LAYERS + 1 entries (the head and every layer, all pending at once: a
//     64-layer model with every layer dropped), and an append past that fails with ERR_RANGES instead of writing.
#pragma once

constexpr int SSAK_MAX_LAYERS = 64;  // ssak_w2v2_config.num_layers (check_config); sizes everything that is per layer
// buffer sets of the queued weight-gradient operands (three: a layer's last product may wait for the launch after next)
constexpr int WGRAD_SETS = 3;

// Launch: int(int n, int tiles) launches the products in slots [0, n), 0 = success.  Announce: void(long offset, long count).
template <class Launch, class Announce>
class WgradSchedule {
 public:
  static constexpr int CAP = 48;  // products in one launch (what ssak_gemm_bf16_grouped takes)
  static constexpr int ROUND_TILES = 256;
  static constexpr int MAX_RANGES = SSAK_MAX_LAYERS + 1;
  static constexpr int ERR_RANGES = -3;  // (= SSAK_ERR_STATE)

  WgradSchedule(Launch launch, Announce announce) : launch_(launch), announce_(announce) {}

  int queued() const { return n_; }
  int queued_tiles() const { return tiles_; }
  int pending_ranges() const { return n_ann_; }
  bool uses_set(int s) const {
    for (int i = 0; i < n_; ++i)
      if (set_[i] == s) return true;
    return false;
  }

  // Queue a product of `tiles` output tiles whose operands live in buffer set `set` (-1: in none); *slot is where the caller
  // keeps its descriptor until the launch.
  int push(int tiles, int set, int* slot) {
    if (n_ > 0 && (tiles_ + tiles > ROUND_TILES || n_ == CAP))
      if (const int rc = flush()) return rc;
    set_[n_] = set;
    tiles_ += tiles;
    ++pushed_;
    *slot = n_++;
    return 0;
  }
  // a layer is about to overwrite set s
  int reserve_set(int s) { return uses_set(s) ? flush() : 0; }
  // launch what is queued, then announce every range at the head of the FIFO that has nothing left to wait for
  int flush() {
    const int rc = n_ > 0 ? launch_(n_, tiles_) : 0;
    launched_ += n_;
    n_ = tiles_ = 0;
    if (rc) return rc;
    drain();
    return 0;
  }
  // the range is complete once the product pushed last has been launched (the lm_head; a kept layer after its qkv product)
  int announce_after_last_product(long off, long cnt) { return append(off, cnt, pushed_ - 1); }
  // the range is complete already (a dropped layer's zeros): now, or behind the ranges still waiting
  int announce_in_order(long off, long cnt) { return append(off, cnt, -1); }

 private:
  struct Range {
    long off, cnt;
    long last;  // sequence number of the range's last product, -1: nothing to wait for
  };
  int append(long off, long cnt, long last) {
    if (n_ann_ == MAX_RANGES) return ERR_RANGES;
    ann_[(head_ + n_ann_++) % MAX_RANGES] = Range{off, cnt, last};
    drain();
    return 0;
  }
  void drain() {
    while (n_ann_ > 0 && ann_[head_].last < launched_) {
      announce_(ann_[head_].off, ann_[head_].cnt);
      head_ = (head_ + 1) % MAX_RANGES;
      --n_ann_;
    }
  }

  Launch launch_;
  Announce announce_;
  int set_[CAP];  // buffer set each queued product reads
  int n_ = 0, tiles_ = 0;
  long pushed_ = 0, launched_ = 0;  // products ever queued / launched
  Range ann_[MAX_RANGES];
  int head_ = 0, n_ann_ = 0;
};
