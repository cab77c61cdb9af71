#!/bin/bash
# Tools-only build (never tracked, never loaded by tests, smoke() or the
# driver): the A/B round forms that tools/valu_microbench.hip times against
# the product's (bit-identical to FIPS 180-4, checked by
# tests/test_rounds_asm_sim.py).
set -euo pipefail
cd "$(dirname "$0")/.."
python3 mirbft_amd/csrc/gen_rounds_asm.py --ab > tools/sha256_rounds_asm_ab.h
echo "tools/sha256_rounds_asm_ab.h generated"
