#!/bin/bash
root=${GRAFT_REPO_ROOT:-/root/repo}
for shape in "4800 512 512" "19200 512 512" "2208 8520 512"; do
  $root/tools/_bin/tgemm_base wgrad $shape
done
