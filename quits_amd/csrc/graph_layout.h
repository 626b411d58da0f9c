// graph_layout.h -- one window's graph laid out for the kernels, on the host alone: every LDS offset, slot order, walk order, bank, dependency
// level and wave map the kernels read (graph_layout.hip).  No HIP header and no device: tests/layout_check.cpp runs it under the sanitizers.
#pragma once
#include "qd_graph_views.h"

#include <cstddef>
#include <memory>
#include <type_traits>
#include <utility>
#include <vector>

#define QD_GEN_PREFIX_LDS (32 * 1024)   // LDS a workgroup of the serial BP kernel may spend on row prefixes (128 slots x 64 shots): five workgroups per CU stay resident

// Sets the message behind qd_last_error and returns `code`.  The library defines it (qd_graph.hip), a test program its own.
int qd_fail(int code, const char *fmt, ...);

// The validation switches of include/quits_amd.h: each selects an alternative that the tests compare bit for bit against the default.
// Read here alone, when a graph or a decoder is created; nothing on the decode path reads the environment.
struct Switches {
    bool no_scatter, scatter_cpl1, scatter_wide_t704, scatter_natural_rounds, scatter_banks_by_slot, scatter_walk_greedy, osdcs_old, bp_no_fast_start;
    float scatter_m2_limit;             // +inf: not set
    std::vector<int> gen_stages;        // iteration bounds between the launches of the serial schedule in the one-message-per-edge kernel
};
Switches qd_read_switches();

// ---- qd_graph_create: qd_host_graph validates the window and derives what the builders share, then qd_layout_graph runs one builder per device
// view, in this order: build_bp (slot orders and BpGraphDev), build_gen (GenGraphDev), build_scatter (ScatGraphDev), build_osd (OsdGraphDev).
struct HostGraph {
    int m = 0, n = 0, nnz = 0, max_rdeg = 0, max_cdeg = 0, min_rdeg = 0, m_pad = 0, n_pad = 0, max_rdeg_pad = 0;
    const int32_t *row_ptr = nullptr, *col_idx = nullptr;
    const double *priors = nullptr;
    std::vector<int> rdeg, cdeg;
    std::vector<double> llr0;                                        // log((1-p)/p), fault order
    std::vector<int32_t> cp, ri, pos;                                // CSC with the edge's position inside its row
    std::vector<int> chk_orig, chk_slot_of, bit_orig, bit_slot_of;   // slots: degree-descending, stable (build_bp)
    std::vector<uint8_t> chk_deg;                                    // [m_pad] degree of the check slot (build_bp)
};
int qd_host_graph(int32_t m, int32_t n, const int32_t *row_ptr, const int32_t *col_idx, const double *priors, HostGraph &h);

// What the builders make: the four views with their pointer members null, and the arrays those members will point at, in the order the
// device receives them.  A staged array names its members by their offset in the image, so whoever uploads (or checks) it needs no list.
struct GraphImage {
    BpGraphDev bp{};
    GenGraphDev gen{};
    OsdGraphDev osd{};
    ScatGraphDev sc{};                 // scatter form of the flooding min-sum kernel (bp_scatter_wide.hip); sc.ok = 0: not for this window
    std::vector<int32_t> h_cp, h_ri;   // host CSC, for the rank
    std::vector<double> h_llr0;        // log((1-p)/p) in double, fault order
    std::vector<uint32_t> h_bit_rec;   // host copy of bp.bit_rec: a decoder on an LLR grid uploads its own with word 0 replaced
    std::vector<uint32_t> h_bit_orig;  // bit slot -> fault
    std::vector<int32_t> h_sc_slot;    // fault -> accumulator slot of the scatter kernels (empty: they are not used)
    long long sc_walk_cycles = 0, sc_walk_ideal = 0;   // modelled LDS cycles of one pass of the scatter kernels' walk, and without any bank conflict
    // Off-chip window: build_bp cannot lay out the gather kernel's LDS state.  bp then holds the shapes and the slot orders alone (threads = lds_bytes = 0),
    // there is no scatter view, BP runs in the one-message-per-edge kernel and OSD-0 in qd_osd0_offchip_kernel.
    bool off_chip = false;

    struct Staged {
        std::unique_ptr<void, void (*)(void *)> owner;   // the builder's own vector, taken over (the deleter knows its type)
        const void *data;
        size_t size;                         // bytes
        std::vector<size_t> fields;          // byte offsets, in the image, of the pointer members that take this array's address
    };
    std::vector<Staged> staged;

    GraphImage() = default;
    GraphImage(const GraphImage &) = delete;
    GraphImage &operator=(const GraphImage &) = delete;

    size_t offset_of(const void *field) const { return (size_t)(static_cast<const unsigned char *>(field) - reinterpret_cast<const unsigned char *>(this)); }
    // Takes the builder's vector over (no copy: the large tables are megabytes per window); an array the builder reads again is staged as a copy.
    template <class Tp, class Fp> void stage(std::vector<Tp> &&h, const Fp **field)
    {
        static_assert(std::is_same<Fp, Tp>::value || std::is_void<Fp>::value, "the member points at another element type");
        auto *own = new std::vector<Tp>(std::move(h));
        staged.push_back({{own, [](void *p) { delete static_cast<std::vector<Tp> *>(p); }}, own->data(), own->size() * sizeof(Tp), {offset_of(field)}});
    }
    template <class Tp, class Fp> void stage(const std::vector<Tp> &h, const Fp **field) { stage(std::vector<Tp>(h), field); }
    template <class Fp> void alias(const Fp **field) { staged.back().fields.push_back(offset_of(field)); }   // a second member for the array staged last
};

int qd_layout_graph(HostGraph &h, const Switches &env, GraphImage *g);
