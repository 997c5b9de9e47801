* resistive divider: onoise = kT4 (R1 || R2) (less the gmin), gain R2 / (R1 + R2)
V1 in 0 DC 1 AC 1
R1 in out 10k
R2 out 0 30k
.NOISE V(out) V1 DEC 5 10 1meg
