#!/bin/bash
# Compare the gfx950 ISA of every kernel (the render objects', rt_comm.o's and the four image passes':
# rt_denoise.o, rt_denoise_samples.o, rt_temporal.o, rt_reproject.o) between a saved snapshot
# and the current build (the instruction text per function: addresses, encodings and branch-target
# labels stripped).  A code change meant to leave the kernels' instruction streams alone must print
# "identical" for them.
# (s_add_u32 / s_addc_u32 literals are PC-relative offsets after s_getpc_b64 -- they move with the
# size of other kernels in the code object -- and are masked.)
# (Zero padding between a function's end and the next function's alignment decodes as
# "v_cndmask_b32_e32 v0, s0, v0, vcc" or "...": such trailing lines are not instructions of the
# function and are dropped, so adding a kernel behind another does not report that one as changed.)
# usage: scripts/isa_compare.sh save DIR | compare DIR
set -eu
B=${ISA_BUILD:-mini-opencl-raytracer_amd/build}  # (ISA_BUILD: a variant's object directory)
LLVM=/opt/rocm/lib/llvm/bin
OBJS="rt_kernels_shipped rt_kernels rt_comm rt_denoise rt_denoise_samples rt_temporal rt_reproject"
dump() {  # dump OUTDIR
  mkdir -p $1
  for o in $OBJS; do
    cp $B/$o.o $1/
    (cd $1 && $LLVM/llvm-objdump --offloading $o.o > /dev/null && mv $o.o.0.hipv4-amdgcn-amd-amdhsa--gfx950 $o.co && rm -f $o.o.0.host* $o.o)
    $LLVM/llvm-objdump -d --no-show-raw-insn $1/$o.co \
      | sed -E 's#[[:space:]]*//.*$##; s/<[^>]*\+0x[0-9a-f]+>//g; s/^(.*s_addc?_u32 .*, )0x[0-9a-f]+$/\1REL/' \
      | awk '/^[0-9a-f]+ <.*>:$/ {name=$2; next} name != "" {$1 = $1; if (NF) print name "\t" $0}' > $1/$o.isa
  done
}
body() {  # body FUNCTION FILE: the function's instruction text without trailing padding
  grep -F "$1" $2 | cut -f2- \
    | awk '{l[NR] = $0} END {n = NR; while (n > 0 && (l[n] == "..." || l[n] == "" || l[n] == "v_cndmask_b32_e32 v0, s0, v0, vcc")) n--; for (i = 1; i <= n; i++) print l[i]}'
}
case $1 in
  save) rm -rf $2; dump $2 ;;
  compare)
    rm -rf /tmp/isa_now
    dump /tmp/isa_now
    for o in $OBJS; do
      for f in $(cut -f1 $2/$o.isa | sort -u); do
        a=$(body "$f" $2/$o.isa | md5sum | cut -c1-12)
        b=$(body "$f" /tmp/isa_now/$o.isa | md5sum | cut -c1-12)
        n=$(grep -cF "$f" /tmp/isa_now/$o.isa || true)
        [ "$a" = "$b" ] && echo "identical  $o $f" || echo "CHANGED    $o $f ($n insts now)"
      done
    done ;;
esac
