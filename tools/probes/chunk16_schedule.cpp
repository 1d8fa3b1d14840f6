// Host replay of conv3x3_chunk_kernel's hand-over schedule (csrc/conv3x3_chunk.hip): no GPU, no HIP.
//
//   c++ -std=c++17 -O1 -o chunk16_schedule tools/probes/chunk16_schedule.cpp && ./chunk16_schedule
//
// The kernel's K loop is replayed per wave with the same control flow: which weight stage every LDS-DMA of a step writes, when the next
// chunk's halo is fetched into registers and when it is stored to the (single) halo buffer, which `s_waitcnt vmcnt(N)` stands in front of
// which barrier, and which stage and halo content the step's fragment reads use.  Time is counted in barriers: barrier 2 s opens K-step
// s = 9 chunk + tap, barrier 2 s + 1 (after tap 8 only) stands in front of the halo stores.  A DMA issued behind barrier g may write its
// LDS bytes at any moment from then until the issuing wave's wait retires it (the queue completes in order: vmcnt(N) retires all but the
// N youngest); a `ds_write` is retired by the `lgkmcnt(0)` in front of the next barrier.  What a wave has retired in front of barrier g is
// visible to every wave behind barrier g.  A wave that has arrived at a barrier has finished the fragment reads in front of it.  For
// 2 ... 7 chunks (and 1, and 12) the program asserts
//   * read after write: the content a step reads was retired by EVERY wave in front of a barrier the reader has passed;
//   * write after read: no write into a stage / the halo buffer is issued while a reader of its previous content can still be in front
//     of the barrier that the writer has passed -- every read of the previous content lies in front of that barrier;
//   * the halo registers of a wave are waited for (by the counted wait of tap 7) before they are stored.
// Deliberately wrong schedules (every wait one DMA short; the halo stored without the barrier of its own; the weights issued one step
// early, into the stage that is being read) must be caught.
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <vector>

namespace {

constexpr int kWaves = 4;
constexpr int ST = 3;        // weight stages
constexpr int LB = 6;        // halo pieces per thread (registers), TH = 8
constexpr int NB = 2;        // weight pieces per wave and stage (the 64-channel tile; 4 for the 128-channel tile: same schedule)
constexpr int kTapLoad = 5;

enum Kind { WEIGHT = 0, HALO = 1 };
struct Write { int kind, buf, content, wave, issue_bar, retire_bar; };      // issued behind barrier issue_bar, retired in front of retire_bar
struct Read { int kind, buf, content, wave, front_bar; };                   // done in front of barrier front_bar (issued behind front_bar - 1 or - 2)

struct Sched { int wait_slack; bool halo_barrier; int weight_early; };      // the kernel: {0, true, 0}

bool replay(int nchunks, Sched sc, bool verbose) {
  std::vector<Write> writes;
  std::vector<Read> reads;
  const int nsteps = 9 * nchunks;
  for (int wave = 0; wave < kWaves; ++wave) {
    struct Op { int write; bool regs; };      // a DMA (index into `writes`) or a register load of the halo
    std::deque<Op> q;                          // this wave's outstanding vector-memory operations, oldest first
    int regs_in_flight = 0;
    auto issue_w = [&](int step, int bar) {
      for (int i = 0; i < NB; ++i) { writes.push_back({WEIGHT, step % ST, step, wave, bar, -1}); q.push_back({(int)writes.size() - 1, false}); }
    };
    auto wait_vmcnt = [&](int n, int bar) {
      while ((int)q.size() > n) {
        if (q.front().regs) --regs_in_flight; else writes[q.front().write].retire_bar = bar;
        q.pop_front();
      }
    };
    auto store_h = [&](int chunk, int behind_bar) -> bool {      // ds_write of the halo registers: retired in front of the next barrier
      if (regs_in_flight) { if (verbose) std::printf("  wave %d stores halo registers of chunk %d that are still in flight\n", wave, chunk); return false; }
      writes.push_back({HALO, 0, chunk, wave, behind_bar, behind_bar + 1});
      return true;
    };
    // prologue: halo registers of chunk 0, the weights of steps 0 ... ST - 2, then the halo stores (the compiler waits for the registers)
    for (int i = 0; i < LB; ++i) { q.push_back({-1, true}); ++regs_in_flight; }
    for (int s = 0; s < ST - 1; ++s) issue_w(s, -1);
    while (regs_in_flight) { if (!q.front().regs) writes[q.front().write].retire_bar = 0; else --regs_in_flight; q.pop_front(); }
    if (!store_h(0, -1)) return false;
    for (int chunk = 0; chunk < nchunks; ++chunk) {
      const bool more = chunk + 1 < nchunks;
      for (int tap = 0; tap < 9; ++tap) {
        const int s = 9 * chunk + tap, bar = 2 * s;
        // ---- the kernel's counted wait, then barrier 2 s ----
        const int ahead = nsteps - 1 - s < ST - 2 ? nsteps - 1 - s : ST - 2;
        wait_vmcnt(ahead * NB + ((tap == kTapLoad + 1 && more) ? LB : 0) + sc.wait_slack, bar);
        // ---- behind it: the issues of the step ----
        if (tap == kTapLoad && more) for (int i = 0; i < LB; ++i) { q.push_back({-1, true}); ++regs_in_flight; }
        const int s2 = s + ST - 1 + sc.weight_early;
        if (s2 < nsteps && (s2 / 9 == chunk || more)) issue_w(s2, bar);
        // ---- the fragment reads of the step: done in front of the next barrier this wave arrives at ----
        const int next_bar = (tap == 8 && more && sc.halo_barrier) ? bar + 1 : bar + 2;
        reads.push_back({WEIGHT, s % ST, s, wave, next_bar});
        reads.push_back({HALO, 0, chunk, wave, next_bar});
      }
      if (more) {
        // barrier 2 s + 1, then the halo stores (the compiler's wait for the registers is not modelled: the counted waits must have retired them)
        const int behind = sc.halo_barrier ? 2 * (9 * chunk + 8) + 1 : 2 * (9 * chunk + 8);
        if (!store_h(chunk + 1, behind)) return false;
      }
    }
    if (!q.empty()) { if (verbose) std::printf("  wave %d leaves %zu operations in flight at the end\n", wave, q.size()); return false; }
  }
  bool ok = true;
  auto fail = [&](const char* what, const Write& w, const Read& r) {
    if (verbose) std::printf("  %s: %s %d, write of content %d by wave %d (behind barrier %d, retired in front of %d) against the read of content %d by wave %d in front of barrier %d\n",
                             what, w.kind == WEIGHT ? "weight stage" : "halo buffer", w.buf, w.content, w.wave, w.issue_bar, w.retire_bar, r.content, r.wave, r.front_bar);
    ok = false;
  };
  for (const Read& r : reads) {
    bool found = false;
    for (const Write& w : writes) {
      if (w.kind != r.kind || w.buf != r.buf) continue;
      // the read is issued behind the barrier that opened its step: the last one before front_bar that is a step barrier
      const int read_behind = r.front_bar % 2 ? r.front_bar - 1 : r.front_bar - 2;
      if (w.content == r.content) {
        found = true;
        if (w.retire_bar < 0 || w.retire_bar > read_behind) fail("read before the data was retired in front of a barrier the reader has passed", w, r);
      } else if (w.content > r.content) {
        // a later content of the same stage / buffer: issued behind a barrier that the reader reaches only with this read done
        if (w.issue_bar < r.front_bar) fail("overwritten while a reader can still be in front of the barrier", w, r);
      }
    }
    if (!found) { if (verbose) std::printf("  a read of content %d that nobody wrote\n", r.content); ok = false; }
  }
  return ok;
}

}  // namespace

int main() {
  int bad = 0;
  for (int nchunks : {1, 2, 3, 4, 5, 6, 7, 12}) {
    const bool ok = replay(nchunks, Sched{0, true, 0}, true);
    std::printf("chunks %2d: %s\n", nchunks, ok ? "ok" : "HAZARD");
    bad += !ok;
  }
  // negative controls: the checker must see these
  for (int nchunks : {2, 3, 7}) {
    if (replay(nchunks, Sched{1, true, 0}, false)) { std::printf("chunks %d: a wait one operation short was NOT caught\n", nchunks); ++bad; }
    if (replay(nchunks, Sched{0, false, 0}, false)) { std::printf("chunks %d: halo stores without their barrier were NOT caught\n", nchunks); ++bad; }
    if (replay(nchunks, Sched{0, true, 1}, false)) { std::printf("chunks %d: weights issued into the stage being read were NOT caught\n", nchunks); ++bad; }
  }
  if (bad) { std::printf("FAILED\n"); return 1; }
  std::printf("schedule ok: no stage or buffer is written while a reader of its previous content can be in front of the barrier\n");
  return 0;
}
