"""Every case of test_device_logic_emulated.py once more, with the wave-per-read program first (GA_LANES=0): <32,false> over all jobs,
then the rungs of graphaligner_amd/csrc/ga_ladder.h.  By the product's rule a batch that starts in the lanes = reads program never
visits <32,false>; this module keeps that variant under every parity case on the host."""
from test_device_logic_emulated import *  # noqa: F401,F403  (the tests, their `lib` fixture and the `first_pass` fixture that reads the name below)

GA_LANES_FIRST = "0"
