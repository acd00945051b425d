// The process-wide rand() read AHEAD without consuming it, for the callers that draw the minimal sets of Sim3Solver::iterate before the device has
// said how many iterations upstream's loop would have run: shells/Sim3Solver.cc (one block of one solver) and Sim3RansacStage
// (PlaceRecognitionStages.h: a window of the stream, drawn once per solver with that solver's N).  Draw on a copy, replay, then move the real
// generator by exactly what upstream would have consumed (rand_advance).  Not thread-safe with respect to other threads calling rand() during the two
// lines that copy the generator state (upstream's use of rand() from several threads is not either).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace rumi_facade {

// glibc's process-wide generator, copied: random_r on the copy gives the values rand() is about to give
struct RandLookahead {
    int32_t table[32];
    char scratch[128], dummy[128];
    struct random_data rd;
    RandLookahead() {
        char *prev = initstate(1u, scratch, sizeof scratch);      // the global generator moves onto `scratch`; glibc returns its own state array,
        std::memcpy(table, prev, sizeof table);                    // word 0 of which now encodes the position it had reached
        setstate(prev);                                            // ... and resumes exactly there
        std::memset(&rd, 0, sizeof rd);
        initstate_r(1u, dummy, sizeof dummy, &rd);
        setstate_r(reinterpret_cast<char *>(table), &rd);
    }
    RandLookahead(const RandLookahead &) = delete;                 // rd points into this object
    RandLookahead &operator=(const RandLookahead &) = delete;
    int next() { int32_t v = 0; random_r(&rd, &v); return (int)v; }
    int RandomInt(int min, int max) { const int d = max - min + 1; return int(((double)next() / ((double)RAND_MAX + 1.0)) * d) + min; }   // DUtils/Random.cpp:47-50
};

// the real generator follows: three draws per iteration upstream really ran (Sim3Solver.cc:249-259)
inline void rand_advance(int iterations) {
    for (int k = 0; k < 3 * iterations; k++) (void)rand();
}

}  // namespace rumi_facade
