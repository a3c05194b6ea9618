#!/bin/bash
# dev experiment: the shader clock k_vocab_f16x3 runs at (a timing build as tools/_bin/libgvl_msda_dev.so; GVL_V_CLOCKS prints
# workgroup 0's cycle and real-time counters)
cd ${GRAFT_REPO_ROOT:-/root/repo}
export GVL_VOCAB_FORM=v
python -m gvl_amd.build --dev gvl_gemm16.hip -DGVL_V_CLOCKS > /dev/null 2>&1
GVL_LIB_PATH=tools/_bin/libgvl_msda_dev.so python tools/vocab_probe.py --time-only --reps 30 2>&1 | grep "round 2\|k_vocab clocks" | tail -4
