// TEST INFRASTRUCTURE ONLY: the launchers of csrc/plume_merkle_launch.h for the CPU build of the library's host side (tests/test_merkle_hostsim.py), in the style of
// host_launch.cpp: a launch queues on the mock runtime's stream a plain loop over the same grid as the kernel (csrc/plume_merkle_kernels.hip), calling the same per-lane
// body (csrc/plume_merkle.h) on the same buffers.  The sort queues one op per kernel of the launcher's own schedule (mrk_sort_schedule); a tile is a heap array.
// One mutant of a LAUNCHER, for the test that shows the driver notices: -DMERKLE_MUTANT_DROPS_STREAM queues k_merkle_place on the null stream instead of the stream it
// was given, so nothing orders it before the levels, the download (host form) or the caller's synchronise (device form).
#include <vector>

#include "plume_merkle_launch.h"

namespace plume {

void launch_merkle_leaf(const MerkleLeafArgs& a0, hipStream_t st) {
    mockhip::launch(st, [a0] { for (uint32_t i = a0.n; i-- > 0;) mrk_leaf_item(a0, i); });
}
void launch_merkle_verify(const MerkleVerifyArgs& a0, hipStream_t st) {
    mockhip::launch(st, [a0] { for (uint32_t i = a0.m; i-- > 0;) mrk_verify_item(a0, i); });
}
void launch_merkle_proof(const MerkleProofArgs& a0, hipStream_t st) {
    mockhip::launch(st, [a0] { for (uint32_t i = a0.m; i-- > 0;) mrk_proof_item(a0, i); });
}
void launch_merkle_place(const MerkleTreeArgs& a0, hipStream_t st) {
#if defined(MERKLE_MUTANT_DROPS_STREAM)
    st = nullptr;
#endif
    mockhip::launch(st, [a0] { for (uint32_t i = a0.n; i-- > 0;) mrk_place_item(a0, i); });
}
void launch_merkle_level(uint8_t* tree, uint32_t n, uint32_t d, hipStream_t st) {
    if (n < 2u || !mrk_depth_nodes(n, d)) return;
    mockhip::launch(st, [tree, n, d] { for (uint32_t t = mrk_depth_nodes(n, d); t-- > 0;) mrk_node(tree, (size_t)mrk_depth_first(d) + t); });
}
void launch_merkle_top(uint8_t* tree, uint32_t n, uint32_t dtop, hipStream_t st) {
    if (n < 2u || dtop > PLUME_MRK_TOP_DEPTH) return;
    mockhip::launch(st, [tree, n, dtop] {
        for (uint32_t d = dtop + 1u; d-- > 0u;)                                            // (the barrier between depths is the loop itself)
            for (uint32_t t = 0; t < 256u; t++) if (t < mrk_depth_nodes(n, d)) mrk_node(tree, (size_t)mrk_depth_first(d) + t);
    });
}
void launch_merkle_sort(const MerkleSortArgs& a0, hipStream_t st) {
    if (!a0.n) return;
    const size_t tiles = a0.npad / a0.tile;
    mrk_sort_schedule(a0.npad, a0.tile,
        [&] {
            mockhip::launch(st, [a0, tiles] {
                std::vector<uint32_t> s((size_t)PLUME_MRK_REC_WORDS * a0.tile);
                for (size_t b = tiles; b-- > 0;) {
                    const size_t base = b * a0.tile;
                    for (uint32_t x = 0; x < a0.tile; x++) mrk_tile_from_leaves(s.data(), a0, base, x);
                    for (uint32_t k = 2; k <= a0.tile; k <<= 1)
                        for (uint32_t j = k >> 1; j; j >>= 1)
                            for (uint32_t t = 0; t < a0.tile / 2u; t++) mrk_tile_cx(s.data(), a0.tile, base, k, j, t);
                    for (uint32_t x = 0; x < a0.tile; x++) mrk_tile_to_ws(s.data(), a0, base, x);
                }
            });
        },
        [&](size_t k, size_t j) { mockhip::launch(st, [a0, k, j] { for (size_t t = a0.npad / 2u; t-- > 0;) mrk_global_cx(a0, k, j, t); }); },
        [&](size_t k) {
            mockhip::launch(st, [a0, tiles, k] {
                std::vector<uint32_t> s((size_t)PLUME_MRK_REC_WORDS * a0.tile);
                for (size_t b = 0; b < tiles; b++) {
                    const size_t base = b * a0.tile;
                    for (uint32_t x = 0; x < a0.tile; x++) mrk_tile_from_ws(s.data(), a0, base, x);
                    for (uint32_t j = a0.tile >> 1; j; j >>= 1)
                        for (uint32_t t = a0.tile / 2u; t-- > 0;) mrk_tile_cx(s.data(), a0.tile, base, k, j, t);
                    for (uint32_t x = 0; x < a0.tile; x++) mrk_tile_to_ws(s.data(), a0, base, x);
                }
            });
        });
}

}  // namespace plume
