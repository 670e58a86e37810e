"""Test infrastructure, never shipped: the CPU restatement of the reference's nine pointnet2 ops (pn2.py,
pn2_oracle.c) and the recipe that compiles the reference's own kernels for gfx950 into oracle/_ref/ as the
bit-for-bit cross-check of that restatement (pn2_ref.py, pn2_ref_glue.cpp, ref_shim/)."""
