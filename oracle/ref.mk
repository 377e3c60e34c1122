# TEST ONLY, included by the Makefile: the reference-side binding (integration/gpu_q_gram_mapper.h) compiled against the
# reference's REAL bucket_map/mapper/mapper.h, found under $(REF).  build() makes it only where that tree is at hand.  The
# program lands in oracle/_ref/, which stays out of git and goes to the GPU machine with the other built files, where
# tests/test_integration_binding.py runs it without the reference.
oracle/_ref/ref_binding: integration/ref_binding_main.cpp integration/gpu_q_gram_mapper.h include/bmf.h $(PKG)/libbmf.so
	mkdir -p oracle/_ref
	$(CXX) -O2 -std=c++17 -Wall -Wextra -o $@ integration/ref_binding_main.cpp -I$(REF)/bucket_map -Iintegration -Iinclude \
	    -L$(PKG) -lbmf -Wl,-rpath,'$$ORIGIN/../../$(PKG)'
