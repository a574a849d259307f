#!/bin/bash
# A/B builds of the library with extra -D flags into build_ab/ (git-ignored; travels to the GPU box): tools/build_ab.sh NAME [-DFLAG ...]
# Compiler flags and source list are the product's (g2048/_build.py).
set -e
ROOT=$(cd $(dirname $0)/.. && pwd)
NAME=$1; shift
mkdir -p $ROOT/build_ab
python3 $ROOT/2048-using-reinforcement-learning_amd/g2048/_build.py -o $ROOT/build_ab/libg2048_$NAME.so "$@" > /dev/null
echo built build_ab/libg2048_$NAME.so "$@"
