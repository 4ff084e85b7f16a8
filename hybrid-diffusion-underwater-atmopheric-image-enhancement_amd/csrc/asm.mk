# `make asm`: the device ISA of every source, with exactly the flags its object is built with (and the mutant sources also with
# the two mutant masks), as text under build/asm/.  -fuse-cuid=none makes the output deterministic.  Included by the Makefile;
# tools/isa_diff.py also hands it (`make -f Makefile -f asm.mk asm`) to a revision whose Makefile predates the target, so the
# flags compared are each revision's own.
ASMFLAGS := -fuse-cuid=none --offload-device-only -S
ASM_DEPS := $(wildcard *.h) ../../include/hdiff.h

build/asm/%.s: %.hip $(ASM_DEPS)
	@mkdir -p $(@D)
	$(HIPCC) $(CXXFLAGS) $(FLAGS_$*) $(ASMFLAGS) $< -o $@
build/asm/mutant/%.s: %.hip $(ASM_DEPS)
	@mkdir -p $(@D)
	$(HIPCC) $(CXXFLAGS) $(FLAGS_$*) -DHDIFF_MUTANT=55 $(ASMFLAGS) $< -o $@
build/asm/mutant2/%.s: %.hip $(ASM_DEPS)
	@mkdir -p $(@D)
	$(HIPCC) $(CXXFLAGS) $(FLAGS_$*) -DHDIFF_MUTANT=72 $(ASMFLAGS) $< -o $@

asm: $(SRCS:%.hip=build/asm/%.s) $(MUT_SRCS:%=build/asm/mutant/%.s) $(MUT2_SRCS:%=build/asm/mutant2/%.s)
.PHONY: asm
