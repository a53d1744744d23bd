#!/bin/bash
# A/B of the `vame` CLI end to end (needs an MI355X): synthetic CSVs once, one
# untimed run that pages them in, then the CLI under each setting, interleaved
# over REPS repetitions.  A setting is "name:VAR=v,...[:binary]": environment
# variables (may be empty) and, optionally, another build of the CLI (a path
# below the repository root; it finds libvame.so through its rpath, so it lies
# in vvc-affine-gpu_amd/bin too).  Each line ends with one digest over the
# names and bytes of the 40 logs the run wrote; a run's stderr (the
# VAME_CLI_TRACE lines) is kept beside its stdout.
#   bash profiles/run_cli_ab.sh <tag> <WxH> <frames> "<name>:<vars>[:<binary>]" ...
# With DISTRUN set to vame.distrun's extra arguments (say "--gpus 2 --rank-only 1")
# the program is `python3 -m vame.distrun $DISTRUN` instead: a setting's third
# field is then the directory that holds the `vame` package to run (another
# commit's, checked out below the repository root; VAME_LIB among the vars points
# it at this tree's library), every setting gets an untimed run of its own, and
# each line adds the timings of the run's DISTRUN record.
set -o pipefail
R="$(cd "$(dirname "$0")/.." && pwd)"
TAG=$1; SIZE=$2; F=$3; shift 3
W=${SIZE%x*}; H=${SIZE#*x}
O=$R/gpurun_out/$TAG; mkdir -p $O
T=$(mktemp -d /tmp/vame_cli.XXXXXX)
trap 'rm -rf $T' EXIT
export PYTHONPATH=$R/vvc-affine-gpu_amd
python3 -c "
from vame.synth import synth_sequence, write_csv
o, r = synth_sequence($W, $H, $F, 32)
write_csv('$T/orig.csv', o); write_csv('$T/recon.csv', r)
" || exit 1
mkdir -p $T/log
for rep in $(seq 0 ${REPS:-2}); do
  for s in "$@"; do
    name=${s%%:*}; rest=${s#*:}; vars=${rest%%:*}
    bin=$R/vvc-affine-gpu_amd/bin/vame
    [[ $rest == *:* ]] && bin=$R/${rest#*:}
    if [ -n "$DISTRUN" ]; then
      pkg=$R/vvc-affine-gpu_amd; [[ $rest == *:* ]] && pkg=$R/${rest#*:}
      bin="env PYTHONPATH=$pkg python3 -m vame.distrun $DISTRUN"
    fi
    rm -f $T/log/*
    env ${vars//,/ } timeout -k 10 300 $bin -f $F -s $SIZE -q 32 -o $T/orig.csv \
        -r $T/recon.csv -l $T/log/x > $O/$name.$rep.txt 2> $O/$name.$rep.err || { echo "$name failed"; exit 1; }
    [ $rep = 0 ] && { echo "$name warm-up done"; [ -n "$DISTRUN" ] && continue; break; }
    echo "$name $rep: $(grep -E 'TOTAL_EXEC|OVERALL|READ_CSV|LOG_WRITE' $O/$name.$rep.txt | tr '\n' ' ')" \
         "$(grep -oE '"(overall|kernel|gpu_gaps|first_frames|read_csv|log_write)_s": [0-9.e-]+' $O/$name.$rep.txt | tr -d '"' | tr '\n' ' ')" \
         "logs $(ls $T/log | wc -l) $(cd $T/log && sha256sum * | sha256sum | cut -c1-16)"
    grep -F '[trace]' $O/$name.$rep.err
  done
done
echo cli-ab-done
