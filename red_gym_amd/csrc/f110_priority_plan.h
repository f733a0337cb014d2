// f110_priority_plan.h -- the host side of the priority tree (f110_priority.h): the level layout of the integer sum tree, the limits
// and the checks every entry point makes before a launch.
// Plain C++17 without HIP (tests/test_priority_cpu.py compiles it for the host); f110_consumers.hip launches what it plans.
// The tree over L leaves (uint32 words): level 1 has ceil(L / 64) uint64 nodes, level k + 1 has ceil(count_k / 64), until a level
// has at most 64 nodes -- the top, whose sum is the total (no root is stored).  With L <= 64 there is no node: the leaves are the top.
// All nodes live in one array, level 1 first.
#pragma once
#include "../../include/f110_hip.h"

#include <cmath>
#include <cstdint>

int fail(int code, const char *fmt, ...);

namespace f110 {

constexpr int PT_FANOUT = 64;                 // children of a node = lanes of a wave
constexpr int PT_MAX_LEVELS = 6;              // node levels of F110_PRIORITY_MAX_LEAVES leaves: 2^25, 2^19, 2^13, 2^7, 2 (5)
constexpr int PT_THREADS = 256;               // 4 waves: 4 nodes, 4 draws or 256 rows of a workgroup

struct PriorityLayout {
    int levels;                               // node levels, 0: the leaves are the top
    long long leaves;
    long long count[PT_MAX_LEVELS];           // nodes of level k + 1
    long long offset[PT_MAX_LEVELS];          // where they start in node[]
    long long words;                          // uint64 words of node[]
};

inline PriorityLayout priority_layout(long long L)
{
    PriorityLayout p = {};
    p.leaves = L;
    long long cur = L;
    while (cur > PT_FANOUT && p.levels < PT_MAX_LEVELS) {
        cur = (cur + PT_FANOUT - 1) / PT_FANOUT;
        p.count[p.levels] = cur;
        p.offset[p.levels] = p.words;
        p.words += cur;
        p.levels++;
    }
    return p;
}

inline bool priority_leaves_ok(long long L) { return L >= 1 && L <= (long long)F110_PRIORITY_MAX_LEAVES; }

// what the stateless entries ask of their tree
inline int priority_tree_check(const char *who, const void *leaf, const void *node, long long L)
{
    if (!priority_leaves_ok(L)) return fail(F110_E_INVALID, "%s: L=%lld leaves (1..%lld)", who, L, (long long)F110_PRIORITY_MAX_LEAVES);
    if (!leaf) return fail(F110_E_INVALID, "%s: null leaf", who);
    if ((uintptr_t)leaf % 4) return fail(F110_E_INVALID, "%s: leaf is not 4-byte aligned", who);
    if (priority_layout(L).words > 0 && !node) return fail(F110_E_INVALID, "%s: null node (L=%lld needs %lld words)", who, L, priority_layout(L).words);
    if ((uintptr_t)node % 8) return fail(F110_E_INVALID, "%s: node is not 8-byte aligned", who);
    return F110_OK;
}

inline int priority_config_check(const char *who, const f110_priority_config *cfg)
{
    if (!cfg) return fail(F110_E_INVALID, "%s: null config", who);
    if (!(cfg->exponent >= 0.0 && cfg->exponent <= 8.0)) return fail(F110_E_INVALID, "%s: exponent %g (0..8)", who, cfg->exponent);
    if (!std::isfinite(cfg->eps) || cfg->eps < 0.0) return fail(F110_E_INVALID, "%s: eps %g (finite, not negative)", who, cfg->eps);
    return F110_OK;
}

// f110_priority_node_words: uint64 words of node[] for L leaves (0 while L <= 64), -1 for an L outside the limits
inline long long priority_node_words(long long L) { return priority_leaves_ok(L) ? priority_layout(L).words : -1; }

} // namespace f110
