// csrc/host_wait.hpp's wait loop with a std::thread in the device's part, built with -fsanitize=thread and run on the CPU
// (tests/test_gpu_ransac_no_events.py).  The "device" writes a four-word record with plain stores and then the sequence word with
// a release store, as k_ransac_finish does behind its system fence; the host waits for the word and reads the record.
//   hand-over   the record read behind the wait is the producer's, 200 times with a new sequence number each
//   stale       the word holds an earlier call's number when the wait begins: the wait does not take it for this batch's
//   silent      the producer ends without writing: the wait returns HOST_WAIT_SILENT and does not hang
//   failed      the producer reports an error: HOST_WAIT_FAILED
// Prints "ok" and exits 0; the sanitiser's own report makes the exit status non-zero.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <thread>
#include "host_wait.hpp"

namespace {
struct Record { int rec[8]; };
std::atomic<int> g_running{0};

void produce(Record* r, int seq, int value, int delay_us, bool write) {
    if (delay_us) std::this_thread::sleep_for(std::chrono::microseconds(delay_us));
    if (write) {
        for (int e = 0; e < 4; ++e) r->rec[e] = value + e;
        __atomic_store_n(&r->rec[4], seq, __ATOMIC_RELEASE);
    }
    g_running.store(0, std::memory_order_release);
}
int producer_state() { return g_running.load(std::memory_order_acquire); }

int fail(const char* what, int a, int b) { std::printf("FAILED %s: %d %d\n", what, a, b); return 1; }
}  // namespace

int main() {
    Record r = {};
    int seq = 0;
    // hand-over, with and without a delay (the word may be there before the first read, or long after the first poll)
    for (int i = 0; i < 200; ++i) {
        ++seq;
        g_running.store(1);
        std::thread t(produce, &r, seq, 1000 * i, i % 4 == 0 ? 300 : 0, true);
        const int st = tdv::wait_for_word(r.rec + 4, seq, producer_state, 20);
        if (st != tdv::HOST_WAIT_OK) { t.join(); return fail("hand-over status", st, i); }
        for (int e = 0; e < 4; ++e) if (r.rec[e] != 1000 * i + e) { t.join(); return fail("hand-over record", r.rec[e], 1000 * i + e); }
        t.join();
    }
    // stale: rec[4] == seq from the last round; the next batch's number is seq + 1 and its producer is slow
    {
        const int stale = seq; ++seq;
        if (r.rec[4] != stale) return fail("stale set-up", r.rec[4], stale);
        g_running.store(1);
        std::thread t(produce, &r, seq, 777, 2000, true);
        const int st = tdv::wait_for_word(r.rec + 4, seq, producer_state, 20);
        const int got = r.rec[0];
        t.join();
        if (st != tdv::HOST_WAIT_OK || got != 777) return fail("stale", st, got);
    }
    // silent: the producer ends and leaves the word alone
    {
        ++seq;
        g_running.store(1);
        std::thread t(produce, &r, seq, 0, 500, false);
        const int st = tdv::wait_for_word(r.rec + 4, seq, producer_state, 20);
        t.join();
        if (st != tdv::HOST_WAIT_SILENT) return fail("silent", st, 0);
    }
    // failed: the producer's state is an error
    {
        ++seq;
        const int st = tdv::wait_for_word(r.rec + 4, seq, [] { return -1; }, 20);
        if (st != tdv::HOST_WAIT_FAILED) return fail("failed", st, 0);
    }
    std::printf("ok\n");
    return 0;
}
