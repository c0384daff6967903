#!/bin/bash
# The octree's timing on one MI355X: every step is a process of its own under its own time limit, and
# a step that fails or runs out of time ends the script. Run from the repository root: bash profiles/time_octree.sh
set -o pipefail
timeout -k 10 120 python profiles/time_octree.py build &&
timeout -k 10 120 python profiles/time_octree.py k20 &&
timeout -k 10 180 python profiles/time_octree.py k40 &&
timeout -k 10 180 python profiles/time_octree.py k100
