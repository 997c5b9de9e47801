* RC low-pass: onoise = kT4 R / (1 + (w R C)^2); its integral over the band is kT / C
V1 in 0 AC 1
R1 in out 1k
C1 out 0 1n
.NOISE V(out,0) V1 DEC 10 1k 100meg
