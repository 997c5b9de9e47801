* RC low-pass for AC analysis: V(out)/V(in) = G / (G + gmin + jwC)
V1 in 0 AC 1
R1 in out 1k
C1 out 0 1n
.AC DEC 10 1k 100meg
