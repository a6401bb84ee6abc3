# tests/ref_link/uci.mk -- TEST INFRASTRUCTURE ONLY: pusch_test on top of the grant-level seam WITH control information (uci_bind.c).
#
# The same link as the `chan` target of the Makefile (the unmodified pusch.o / pdsch.o / sch.o with their four definitions renamed to <name>_ref), with
# uci_bind.c in chan_bind.c's place: it includes chan_bind.c whole and adds the PUSCH grants that carry HARQ-ACK / RI / CQI bits.
#   make -C tests/ref_link -f uci.mk uci
include Makefile

UCI_PROGS = pusch_test
UCI_BINS  = $(addprefix $(OUT)/bin_uci/,$(UCI_PROGS))

$(OUT)/obj/uci/uci_bind.o: uci_bind.c chan_bind.c
	@mkdir -p $(dir $@)
	$(CC) $(CFLAGS) -Wall -Wno-unused-function -c uci_bind.c -o $@

$(UCI_BINS): $(OUT)/bin_uci/%: $(OUT)/bin_full/% $(OUT)/obj/tb/tb_bind.o $(OUT)/obj/tb/tb_tx_bind.o $(OUT)/obj/uci/uci_bind.o $(OUT)/libsrsran_phy_rest_chan.a
	@mkdir -p $(dir $@)
	$(CXX) -o $@ $(OUT)/obj/full/$(notdir $@).o $(OUT)/obj/tb/tb_bind.o $(OUT)/obj/tb/tb_tx_bind.o $(OUT)/obj/uci/uci_bind.o $(OUT)/libsrsran_phy_rest_chan.a \
	  -L$(ROOT)/srslte_amd/lib -lsrsran_phy_hip -Wl,-rpath,'$$ORIGIN/../../../../srslte_amd/lib' -lpthread -lm

uci: $(UCI_BINS)

.PHONY: uci
