* series RLC driven by an AC source
V1 in 0 DC 0 AC 1
R1 in a 50
L1 a b 1u
C1 b 0 1n
.AC LIN 41 1meg 11meg
