// TEST INFRASTRUCTURE ONLY: the launchers of csrc/plume_eth_tx_sign_launch.h for the CPU build of the library's host side (tests/test_eth_tx_sign_hostsim.py), in the style
// of host_launch.cpp: a launch queues on the mock runtime's stream a plain loop over the same grid as the kernel (csrc/plume_eth_tx_sign_kernels.hip), calling the same
// per-lane body (csrc/plume_eth_tx_sign.h) on the same buffers.  Lanes run last-to-first.
// One mutant of the LAUNCHER, for the test that shows the driver notices: -DETH_TX_SIGN_MUTANT_WRITES_PAST lets the assemble write one byte past out_len of every signed item
// whose slot has room for it.
#include "plume_eth_tx_sign_launch.h"

namespace plume {

void launch_eth_tx_sign_frame(const EthTxSignArgs& a0, hipStream_t st) {
    if (!a0.n) return;
    mockhip::launch(st, [a0] { for (uint32_t i = a0.n; i-- > 0;) eth_tx_sign_frame_item(a0, i); });
}
void launch_eth_tx_sign_assemble(const EthTxSignArgs& a0, hipStream_t st) {
    if (!a0.n) return;
    mockhip::launch(st, [a0] {
        for (uint32_t i = a0.n; i-- > 0;) {
            eth_tx_sign_assemble_item(a0, i);
#if defined(ETH_TX_SIGN_MUTANT_WRITES_PAST)
            const uint64_t slot_len = a0.tx_off[i + 1] - a0.tx_off[i] + PLUME_ETHTXK_SIGN_GROWTH;
            if (a0.status[i] == 0 && a0.out_len[i] < slot_len) a0.out[(a0.tx_off[i] - a0.tx_off[0]) + (uint64_t)PLUME_ETHTXK_SIGN_GROWTH * i + a0.out_len[i]] = 0x5A;
#endif
        }
    });
}

}  // namespace plume
