# Build of the product library (HIP kernels + C ABI) and of the test oracle.
#   make            -> generalized_rbda_amd/libgrbda_hip.so, oracle/_build/libgrbda_oracle.so
#   make ref        -> oracle/_ref/libgrbda_codegen_ref.so (needs /root/reference; see oracle/Makefile)
HIPCC ?= hipcc
ARCH  ?= gfx950
CSRC  := generalized_rbda_amd/csrc
OBJ   := build/obj
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-function
# the SLP vectoriser pairs fp32 operations into v_pk_* instructions and pays for it in register moves
# (measured: 6-10% slower f32 ABA); the kernels are scalar-per-lane code
KERNFLAGS := -fno-slp-vectorize

LIB := generalized_rbda_amd/libgrbda_hip.so

all: $(LIB) oracle

$(OBJ)/kernels.o: $(CSRC)/kernels.hip $(CSRC)/plan.h $(CSRC)/devplan.h $(CSRC)/devmath.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(KERNFLAGS) -c $< -o $@
# The chain kernels may re-associate sums (no signed zeros, no traps; NOT reciprocal / finite-math-only / approximate
# functions): lone multiplies and adds of the spatial products fold into FMAs, 10 % fewer floating-point instructions
# (MIT humanoid fp32 ABA 0.173 -> 0.170 ms, JVRC-1 and TelloWithArms 3-4 %); parity tolerances unchanged.
CHAINFLAGS := -fassociative-math -fno-signed-zeros -fno-trapping-math
$(OBJ)/chain_kernels.o: $(CSRC)/chain_kernels.hip $(CSRC)/gen_segments.h $(CSRC)/gen_rnea_segments.h $(CSRC)/plan.h $(CSRC)/devplan.h $(CSRC)/devmath.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(KERNFLAGS) $(CHAINFLAGS) -c $< -o $@
# second unit of the same source: the two fp64 kernels with the deepest register pressure (see the head of chain_kernels.hip)
$(OBJ)/chain_kernels_u1.o: $(CSRC)/chain_kernels.hip $(CSRC)/gen_segments.h $(CSRC)/gen_rnea_segments.h $(CSRC)/plan.h $(CSRC)/devplan.h $(CSRC)/devmath.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(KERNFLAGS) $(CHAINFLAGS) -DGRBDA_CHAIN_UNIT=1 -c $< -o $@
# third unit: the kernels of chain programs with generic clusters (gen_segments.h)
$(OBJ)/chain_kernels_u2.o: $(CSRC)/chain_kernels.hip $(CSRC)/gen_segments.h $(CSRC)/gen_rnea_segments.h $(CSRC)/plan.h $(CSRC)/devplan.h $(CSRC)/devmath.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(KERNFLAGS) $(CHAINFLAGS) -DGRBDA_CHAIN_UNIT=2 -c $< -o $@
# fourth unit: the latency-mode kernel with four wavefronts per tile (its [K | y0] blocks are LDS objects: GRBDA_KLDS)
$(OBJ)/chain_kernels_u3.o: $(CSRC)/chain_kernels.hip $(CSRC)/gen_segments.h $(CSRC)/gen_rnea_segments.h $(CSRC)/plan.h $(CSRC)/devplan.h $(CSRC)/devmath.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(KERNFLAGS) $(CHAINFLAGS) -DGRBDA_CHAIN_UNIT=3 -c $< -o $@
# fifth unit: the wrench-carrying chain kernels (include/grbda_hip_wrench.h), kept away from every other kernel's code generation
$(OBJ)/chain_kernels_u4.o: $(CSRC)/chain_kernels.hip $(CSRC)/gen_segments.h $(CSRC)/gen_rnea_segments.h $(CSRC)/plan.h $(CSRC)/devplan.h $(CSRC)/devmath.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(KERNFLAGS) $(CHAINFLAGS) -DGRBDA_CHAIN_UNIT=4 -c $< -o $@
$(OBJ)/wrench_kernels.o: $(CSRC)/wrench_kernels.hip $(CSRC)/plan.h $(CSRC)/devplan.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(KERNFLAGS) -c $< -o $@
# poses and twists of a listed few bodies (include/grbda_hip_bodies.h)
$(OBJ)/body_list_kernels.o: $(CSRC)/body_list_kernels.hip $(CSRC)/plan.h $(CSRC)/devplan.h $(CSRC)/devmath.h $(CSRC)/walk.h $(CSRC)/walk_dev.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(KERNFLAGS) -c $< -o $@
# frame Jacobians and their drift at a listed few body frames (include/grbda_hip_jacobians.h)
$(OBJ)/frame_jacobian_kernels.o: $(CSRC)/frame_jacobian_kernels.hip $(CSRC)/plan.h $(CSRC)/devplan.h $(CSRC)/devmath.h $(CSRC)/walk.h $(CSRC)/walk_dev.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(KERNFLAGS) -c $< -o $@
# J v and J^T f at a listed few body frames, J never formed (include/grbda_hip_jacobian_products.h)
$(OBJ)/frame_product_kernels.o: $(CSRC)/frame_product_kernels.hip $(CSRC)/plan.h $(CSRC)/devplan.h $(CSRC)/devmath.h $(CSRC)/walk.h $(CSRC)/walk_dev.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(KERNFLAGS) -c $< -o $@
$(OBJ)/crba_kernels.o: $(CSRC)/crba_kernels.hip $(CSRC)/plan.h $(CSRC)/devplan.h $(CSRC)/devmath.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(KERNFLAGS) -c $< -o $@
$(OBJ)/deriv_kernels.o: $(CSRC)/deriv_kernels.hip $(CSRC)/plan.h $(CSRC)/devplan.h $(CSRC)/devmath.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(KERNFLAGS) -c $< -o $@
$(OBJ)/minv_kernels.o: $(CSRC)/minv_kernels.hip $(CSRC)/plan.h $(CSRC)/devplan.h $(CSRC)/devmath.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(KERNFLAGS) -c $< -o $@
$(OBJ)/manifold_kernels.o: $(CSRC)/manifold_kernels.hip $(CSRC)/plan.h $(CSRC)/devplan.h $(CSRC)/devmath.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(KERNFLAGS) -c $< -o $@
$(OBJ)/contact_kernels.o: $(CSRC)/contact_kernels.hip $(CSRC)/plan.h $(CSRC)/devplan.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(KERNFLAGS) -c $< -o $@
# the solve of the scheduled contacts (include/grbda_hip_contact_step.h)
$(OBJ)/contact_step_kernels.o: $(CSRC)/contact_step_kernels.hip $(CSRC)/plan.h $(CSRC)/devplan.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(KERNFLAGS) -c $< -o $@
$(OBJ)/centroidal_kernels.o: $(CSRC)/centroidal_kernels.hip $(CSRC)/plan.h $(CSRC)/devplan.h $(CSRC)/devmath.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(KERNFLAGS) -c $< -o $@
$(OBJ)/vjp_kernels.o: $(CSRC)/vjp_kernels.hip $(CSRC)/plan.h $(CSRC)/devplan.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(KERNFLAGS) -c $< -o $@
$(OBJ)/jvp_kernels.o: $(CSRC)/jvp_kernels.hip $(CSRC)/plan.h $(CSRC)/devplan.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(KERNFLAGS) -c $< -o $@
$(OBJ)/step_vjp_kernels.o: $(CSRC)/step_vjp_kernels.hip $(CSRC)/plan.h $(CSRC)/devplan.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) $(KERNFLAGS) -c $< -o $@
$(OBJ)/capi.o: $(CSRC)/capi.cpp $(CSRC)/plan.h $(CSRC)/devplan.h $(CSRC)/walk.h include/grbda_hip.h include/grbda_hip_vjp.h include/grbda_hip_step_vjp.h include/grbda_hip_jvp.h include/grbda_hip_wrench.h include/grbda_hip_contact_step.h include/grbda_hip_bodies.h include/grbda_hip_jacobians.h include/grbda_hip_jacobian_products.h include/grbda_model_desc.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@
$(OBJ)/plan.o: $(CSRC)/plan.cpp $(CSRC)/plan.h include/grbda_hip.h include/grbda_model_desc.h
	@mkdir -p $(OBJ)
	g++ -O2 -std=c++17 -fPIC -Wall -c $< -o $@
# the ancestor walks of the listed-body and frame-Jacobian paths: plain C++ like the plan compiler (make asan drives it too)
$(OBJ)/walk.o: $(CSRC)/walk.cpp $(CSRC)/walk.h $(CSRC)/plan.h
	@mkdir -p $(OBJ)
	g++ -O2 -std=c++17 -fPIC -Wall -c $< -o $@
$(OBJ)/urdf.o: $(CSRC)/urdf.cpp include/grbda_hip.h include/grbda_model_desc.h generalized_rbda_amd/include/grbda/ModelDescription.h
	@mkdir -p $(OBJ)
	g++ -O2 -std=c++17 -fPIC -Wall -c $< -o $@

$(LIB): $(OBJ)/kernels.o $(OBJ)/chain_kernels.o $(OBJ)/chain_kernels_u1.o $(OBJ)/chain_kernels_u2.o $(OBJ)/chain_kernels_u3.o $(OBJ)/chain_kernels_u4.o $(OBJ)/wrench_kernels.o $(OBJ)/body_list_kernels.o $(OBJ)/frame_jacobian_kernels.o $(OBJ)/frame_product_kernels.o $(OBJ)/crba_kernels.o $(OBJ)/deriv_kernels.o $(OBJ)/minv_kernels.o $(OBJ)/manifold_kernels.o $(OBJ)/contact_kernels.o $(OBJ)/contact_step_kernels.o $(OBJ)/centroidal_kernels.o $(OBJ)/vjp_kernels.o $(OBJ)/jvp_kernels.o $(OBJ)/step_vjp_kernels.o $(OBJ)/capi.o $(OBJ)/plan.o $(OBJ)/walk.o $(OBJ)/urdf.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

oracle:
	$(MAKE) -C oracle

ref:
	$(MAKE) -C oracle ref

clean:
	rm -rf build $(LIB) oracle/_build oracle/_ref

.PHONY: all oracle ref clean

# AddressSanitizer + UBSan build of the HOST-side code (CPU only: GPU sanitizers are not available on this pool): the plan
# compiler, the walk builders, the URDF+ reader and the oracle, driven by tools/asan_driver.cpp over every robot URDF and a serialised model.
#   make asan && build/asan/asan_driver tests/golden/robot-models/*.urdf
asan:
	@mkdir -p build/asan
	g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -Wall \
	    -DGRBDA_ASAN_DRIVER -I include -I generalized_rbda_amd/include tools/asan_driver.cpp $(CSRC)/plan.cpp $(CSRC)/walk.cpp $(CSRC)/urdf.cpp \
	    -x c oracle/grbda_oracle.c -x none -lm -lpthread -o build/asan/asan_driver
.PHONY: asan

# host-side checker of the chain programs' LDS / slab schedules against the kernels' accesses (tests/test_lds_schedule_cpu.py)
#   make lds-check && build/lds_check/lds_schedule_check --self-test tests/golden/robot-models/*.urdf
lds-check:
	@mkdir -p build/lds_check
	g++ -std=c++17 -O1 -g -Wall -I include -I generalized_rbda_amd/include tests/cpp/lds_schedule_check.cpp $(CSRC)/plan.cpp \
	    $(CSRC)/urdf.cpp -o build/lds_check/lds_schedule_check
.PHONY: lds-check

# host-side check of the chain forward dynamics' slab rule (devplan.h, chain_slab_rows) over the plans of real robots, under
# AddressSanitizer + UBSan (host code only; tests/test_chain_slab_rule_cpu.py)
#   make slab-check && build/slab_check/chain_slab_check tests/golden/robot-models/*.urdf
slab-check:
	@mkdir -p build/slab_check
	$(HIPCC) -x hip --cuda-host-only -std=c++17 -O1 -g -Wall -Wno-unused-function -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
	    -I include -I generalized_rbda_amd/include tests/cpp/chain_slab_check.cpp $(CSRC)/plan.cpp $(CSRC)/urdf.cpp \
	    -fsanitize=address,undefined -o build/slab_check/chain_slab_check
.PHONY: slab-check
