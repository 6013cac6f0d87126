// TEST INFRASTRUCTURE ONLY: the launcher of csrc/plume_eth_tx_launch.h for the CPU build of the library's host side (tests/test_eth_tx_hostsim.py), in the style of
// host_launch.cpp: a launch queues on the mock runtime's stream a plain loop over the same grid as k_eth_tx_parse (csrc/plume_eth_tx_kernels.hip), calling the same
// per-lane body (csrc/plume_eth_tx.h) on the same buffers.  Lanes run last-to-first.
// One mutant of the LAUNCHER, for the test that shows the driver notices: -DETH_TX_MUTANT_DROPS_STREAM queues the loop on the null stream instead of the stream it was
// given, so nothing orders it before the recover stages, the download (host form) or the caller's synchronise (device form).
#include "plume_eth_tx_launch.h"

namespace plume {

void launch_eth_tx_parse(const EthTxArgs& a0, hipStream_t st) {
#if defined(ETH_TX_MUTANT_DROPS_STREAM)
    st = nullptr;
#endif
    mockhip::launch(st, [a0] {
        for (uint32_t i = a0.n; i-- > 0;) eth_tx_parse_item(a0, i);
    });
}

}  // namespace plume
