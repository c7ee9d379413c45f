// What node_attention.hip (forward, and its training form that also leaves the softmax statistics) and node_attention_bwd.hip (backward)
// share: the constants of the lane mapping and of the two-level sum, and ONE copy of the score, so that the backward's recomputed weight
// exp2((s - m) * log2e) * inv_den goes through the very operations of the forward's.
#pragma once
#include "common.h"

namespace gnnome {

constexpr int kAttThreads = 256;
constexpr int kAttHeads = 3;
constexpr int kAttHubThreshold = 4096;   // items above which a list is summed in two levels
constexpr int kAttHubBlock = 128;        // items per first-level block of such a list (a multiple of the 64-item batch)
constexpr int kAttInFlight = 4;          // rows (three 16-byte requests each) per lane group in flight
constexpr float kLog2e = 1.4426950408889634f;
constexpr int kAttStatsRow = 8;          // floats per node of the statistics: m0 m1 m2 0 | 1/den0 1/den1 1/den2 0

struct AttScores {   // per head
    float v[kAttHeads];
};

// leaky_relu(el + er) per head; a NaN stays a NaN (NaN > 0 is false, slope * NaN is NaN)
__device__ __forceinline__ AttScores att_scores(const f32x4 el, const AttScores& er, float slope) {
    AttScores s;
#pragma unroll
    for (int k = 0; k < kAttHeads; ++k) {
        const float x = el[k] + er.v[k];
        s.v[k] = x > 0.f ? x : slope * x;
    }
    return s;
}

}  // namespace gnnome
