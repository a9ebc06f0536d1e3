// The host's wait for a word that a producer - a kernel's last store into fine-grained pinned memory (ransac.hip: k_ransac_finish's
// sequence word), or a thread in tests/csrc/record_wait_tsan.cpp - sets once everything it hands over has been written.
// No HIP here: what "the producer" is comes in as a callable, so that the loop can be built and run under -fsanitize=thread
// on a machine without a device.
#pragma once
#include <chrono>

namespace tdv {

enum { HOST_WAIT_OK = 0, HOST_WAIT_FAILED = 1, HOST_WAIT_SILENT = 2 };   // the word came; the producer reports an error; it ended and left the word unset

inline void cpu_pause() {
#if (defined(__x86_64__) || defined(__i386__)) && !defined(__HIP_DEVICE_COMPILE__)
    __builtin_ia32_pause();
#elif defined(__aarch64__) && !defined(__HIP_DEVICE_COMPILE__)
    asm volatile("yield");
#endif
}

// Spins on an acquire load of *word until it reads `want`: what the producer wrote before its release store of the word is visible
// behind the return.  The spin cannot hang on a producer that died: every poll_us microseconds of the host's clock it asks
// producer() - > 0 still running, 0 ended, < 0 failed.  A producer that has ended gets one more read of the word (its store may
// have landed between the last read and the question); still unset, the wait ends with HOST_WAIT_SILENT.
template <class Producer>
inline int wait_for_word(const volatile int* word, int want, Producer&& producer, int poll_us = 50) {
    using clock = std::chrono::steady_clock;
    const int* const w = const_cast<const int*>(word);
    clock::time_point last = clock::now();
    for (unsigned spins = 1;; ++spins) {
        if (__atomic_load_n(w, __ATOMIC_ACQUIRE) == want) return HOST_WAIT_OK;
        cpu_pause();
        if (spins % 32u) continue;               // the clock itself every 32 reads
        const clock::time_point now = clock::now();
        if (now - last < std::chrono::microseconds(poll_us)) continue;
        last = now;
        const int state = producer();
        if (state > 0) continue;
        if (state < 0) return HOST_WAIT_FAILED;
        return __atomic_load_n(w, __ATOMIC_ACQUIRE) == want ? HOST_WAIT_OK : HOST_WAIT_SILENT;
    }
}

}  // namespace tdv
